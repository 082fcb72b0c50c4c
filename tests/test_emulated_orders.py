"""CPU tests (no GPU): the rows of tests/order_cases.py which the wavefront emulator can run (tests/emu: the cluster kernels
and the staged table stepper, not the stepper with events), at Taylor orders other than 20 - one step of 2 S + 3 systems
with all Taylor coefficients against the oracle at the tolerances of tests/test_emulated_kernels.py, batch-size independence
in every row, and for the one-lane-per-pair kernel the propagation through the work queue with refill at orders 3 and
22. The hardware's side - LDS sizes, spilling builds, the kernels behind the stepper - is tests/test_orders_gpu.py.

The pools are the well conditioned ones of tests/test_emulated_kernels.py (clouds of bodies, the outer Solar System perturbed
by 1e-6), not the ring pools of the GPU families: on the ring pool of model::nbody(3) the step sizes of kernel and oracle
differ by up to 8.9e3 eps at order 28 with the coefficients agreeing to 3e2 eps - the conditioning of the selector on that
pool. On the pools here the oracle's own two orders of the operations (default and compact mode) agree to 2 eps on h and
420 eps on the state at every order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import emu  # noqa: E402
import heyoka_oracle as ho  # noqa: E402

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402
from heyoka_amd import mixed_models as mm  # noqa: E402

import order_cases as oc  # noqa: E402
from test_emulated_kernels import EPS, rel_err  # noqa: E402


def _cloud(nb):
    """The states of test_emulated_v5_other_systems_single_step_vs_oracle."""
    def state(n):
        rng = np.random.RandomState(40 + nb)
        pos = rng.uniform(-3.0, 3.0, (nb, 3, n)) + 6.0 * np.arange(nb)[:, None, None] * np.array([1.0, 0.3, -0.2])[None, :, None]
        vel = rng.uniform(-0.3, 0.3, (nb, 3, n))
        return np.concatenate([np.concatenate([pos[b], vel[b]], axis=0) for b in range(nb)], axis=0)
    return state


def _outer(n):
    return configs.outer_ss_state(n, perturb=1e-6, seed=5)


def _np1body(n):
    full = _outer(n).reshape(6, 6, n)
    return np.ascontiguousarray((full[1:] - full[:1]).reshape(30, n))


# family -> (pool, horizon of the propagation through the work queue: the one-lane-per-pair kernels)
_POOLS = {
    "v5": (_outer, 4.0), "v5_32_lanes": (_cloud(8), 6.0), "v5_8_lanes_lds_jets": (_cloud(3), 6.0), "v5_16_lanes_lds_jets": (_cloud(4), 6.0),
    "v3": (_outer, None), "v3_64_lanes": (_cloud(7), None), "v2": (_outer, None), "v2_aliased": (_np1body, None),
    "multi_class": (lambda n: mm.sine_lattice_state(16, n), None), "staged": (_outer, None),
}

# (case of ORDER_CASES, variant). Variants: "" - the family as it is; "nofrx" - the one-lane-per-pair kernel in the layout the
# stepper with events keeps (reactions exported by the pair lanes, 128-bit operand reads), at the odd and the high order;
# "compact" - the staged stepper with kw::compact_mode, the strict order of the additions.
ROWS = [(c, "") for c in oc.ORDER_CASES if c[0] in _POOLS]
ROWS += [(c, "nofrx") for c in oc.cases_of("v5") if c[1] in (3, 22)]
ROWS += [(c, "compact") for c in oc.cases_of("staged")]


def _row_id(row):
    return oc.case_id(row[0]) + ("-" + row[1] if row[1] else "")


def _build(case, variant):
    family, order = case[0], case[1]
    kw, okw = {}, dict(oc.family_of(family).get("okw", {}))
    if variant == "compact":
        kw["compact_mode"] = True
    if family == "staged":
        # (Both settings of the staged stepper are held to the COMPACT-mode oracle, as in tests/test_emulated_kernels.py.)
        okw["compact_mode"] = True
    with oc._env({"HEYOKA_AMD_V5_OPTS": "nofrx"} if variant == "nofrx" else None):
        ta = oc.construct(family, order, **kw)
    oc.check_mode(case, ta.hip_source_mode)
    if variant == "nofrx":
        assert "const hy_d2 w" in ta.hip_source  # (128-bit operand reads: only in the nofrx layout)
    if variant == "compact":
        assert "strict order" in ta.hip_source_mode
    return ta, okw


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_emulated_order_cases_single_step_vs_oracle(row):
    """One step of 2 S + 3 systems (S: the systems of a wavefront or workgroup; the last wavefront is ragged) with all
    Taylor coefficients: step sizes to 1e4 eps, states and coefficients (rows scaled by their maximum over the systems) to
    1e5 eps of the oracle's; the multi-class stepper's coefficients the default-mode oracle's and the staged stepper's with
    kw::compact_mode the compact-mode oracle's BIT FOR BIT. In every row - every kernel and layout at each of its orders, the
    kernels which index a.scratch by their wavefront included -: batches of 1, 2, 3, S - 1, S and S + 1 systems and a window
    of the large run bit for bit its columns. The rows with the jets in global scratch run on a scratch buffer sized from
    the integrator's scratch_per_wave, as the host driver's."""
    case, variant = row
    family, order = case[0], case[1]
    ta, okw = _build(case, variant)
    p = ta.order
    assert p == order
    S = oc.systems_per_unit(ta.hip_source_mode)
    n = 2 * S + 3
    st = _POOLS[family][0](n)
    dim = st.shape[0]
    k = emu.EmulatedKernel(ta.hip_source, scratch_per_wave=ta.scratch_per_wave)
    assert (ta.scratch_per_wave > 0) == ("jets in global scratch" in ta.hip_source_mode) == k.reads_scratch
    rows = dim * (p + 1)
    big = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows)
    ora = ho.OracleIntegrator(oc.family_of(family)["sys"](ho), st, n, tol=oc.tol_for_order(order), **okw)
    assert ora.order == p
    ora.step(wtc=True)
    h_o = np.array([h for _, h in ora.step_res])
    tc_o = ora.tc.reshape(dim, p + 1, n)
    tc = big["tc"].reshape(tc_o.shape)
    scale = np.max(np.abs(tc_o), axis=2, keepdims=True) + 1e-300
    e_h, e_st = rel_err(big["last_h"], h_o) / EPS, rel_err(big["state"], ora.state.reshape(dim, n)) / EPS
    e_tc = float(np.max(np.abs(tc - tc_o) / scale)) / EPS
    print("\n[%s, emulated, eps] h %.3g, state %.3g, Taylor coefficients %.3g (S = %d, %d systems)" % (_row_id(row), e_h, e_st, e_tc, S, n))
    assert np.all(big["last_h"] > 0) and np.isfinite(tc).all()
    assert e_h <= 1e4 and e_st <= 1e5 and e_tc <= 1e5
    assert rel_err(big["time_hi"], ora.time_hi) <= 1e4 * EPS
    if family == "multi_class" or variant == "compact":
        assert np.array_equal(tc, tc_o)
    for idx in [np.arange(m) for m in sorted({1, 2, 3, S - 1, S, S + 1} - {0})] + [np.arange(3, 3 + S + 1)]:
        m = len(idx)
        part = k.run(st[:, idx], np.zeros(m), np.zeros(m), mode=0, lim=np.full(m, np.inf), want_tc_rows=rows)
        for key in ("state", "time_hi", "time_lo", "last_h", "outcome", "tc"):
            assert np.array_equal(part[key], big[key][..., idx]), (_row_id(row), key, "systems %d .. %d" % (idx[0], idx[-1]))


@pytest.mark.parametrize("case", [c for c in oc.ORDER_CASES if c[0] in _POOLS and _POOLS[c[0]][1] is not None and c[1] in (3, 22)], ids=oc.case_id)
def test_emulated_v5_work_queue_with_refill_at_other_orders(case):
    """propagate_until() with per-system final times through ONE workgroup, 5 systems more than it keeps in flight: the
    retire / refill path of the one-lane-per-pair kernel at orders 3 and 22. Outcomes and final times exact, step counts
    within 1 of the oracle's, states to 1e5 eps."""
    family, order = case[0], case[1]
    ta, okw = _build(case, "")
    assert "snew < N" in ta.hip_source  # (this kernel has the refill path)
    state, horizon = _POOLS[family]
    k = emu.EmulatedKernel(ta.hip_source, scratch_per_wave=ta.scratch_per_wave)
    n = k.block // k.lanes_per_system + 5
    st = state(n)
    tf = horizon * np.random.RandomState(3).uniform(0.2, 1.5, n)
    r = k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=tf, max_grid=1)
    ora = ho.OracleIntegrator(oc.family_of(family)["sys"](ho), st, n, tol=oc.tol_for_order(order), **okw)
    ora.propagate_until(tf)
    ns_o = np.array([int(q[3]) for q in ora.prop_res])
    dn = np.abs(r["n_steps"].astype(np.int64) - ns_o)
    e_st = rel_err(r["state"], ora.state.reshape(st.shape[0], n)) / EPS
    print("\n[%s, emulated work queue] %d systems, %d .. %d steps, %d step counts differ, state %.3g eps" % (oc.case_id(case), n, ns_o.min(), ns_o.max(),
                                                                                                        np.count_nonzero(dn), e_st))
    assert np.array_equal(r["outcome"], np.array([int(q[0]) for q in ora.prop_res]))
    assert np.array_equal(r["time_hi"], tf)
    assert dn.max() <= 1
    assert e_st <= 1e5


def test_emulated_kernel_refuses_to_run_without_its_jet_scratch():
    """A kernel with the jets in global scratch: the emulator sizes a.scratch from the integrator's scratch_per_wave, as
    the host driver does; without it, or with a figure smaller than the module's, run() raises (a null a.scratch used to
    be dereferenced, and the interpreter died)."""
    case = [c for c in oc.cases_of("v3") if c[1] == 26][0]
    ta, _ = _build(case, "")
    # (The jets of a wavefront: [order + 1][systems of the wavefront][columns].)
    assert ta.scratch_per_wave >= 27 * 2 * 36
    assert oc.construct("v3", 22).scratch_per_wave == 0  # (jets in LDS)
    n = 3
    st = _outer(n)
    k = emu.EmulatedKernel(ta.hip_source, scratch_per_wave=ta.scratch_per_wave)
    with pytest.raises(ValueError, match="module reports"):
        k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), scratch_per_wave=ta.scratch_per_wave - 1)
    k = emu.EmulatedKernel(ta.hip_source)
    assert k.reads_scratch
    with pytest.raises(ValueError, match="scratch_per_wave"):
        k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf))
