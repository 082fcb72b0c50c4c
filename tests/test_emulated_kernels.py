"""CPU tests (no GPU): the generated stepper kernels, compiled for the HOST and run under the wavefront emulator of
tests/emu (fibres with rendezvous at the cross-lane operations), against the oracle. TEST INFRASTRUCTURE: the emulator is
a checker of the generators' arithmetic and exchange logic in the authoring container - the proof for the hardware stays
with the -m gpu parity tests, which run the same comparisons through the C ABI on an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import emu  # noqa: E402
import heyoka_oracle as ho  # noqa: E402

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

EPS = 2.220446049250313e-16
M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-300)))


def _outer_ss(kernel, monkeypatch=None, **kw):
    # ("v5-nofrx": the one-lane-per-pair kernel with the reactions exported by the pair lanes and the consumer-arranged
    # operand arrays read with 128-bit loads - the layout the stepper with events keeps.)
    opts = None
    if kernel.endswith("-nofrx"):
        kernel, opts = kernel[:-6], "nofrx"
    old = os.environ.get("HEYOKA_AMD_V5_OPTS")
    if opts is not None:
        os.environ["HEYOKA_AMD_V5_OPTS"] = opts
    try:
        ta = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), None, 64, high_accuracy=True, cluster_kernel=kernel, **kw)
    finally:
        if opts is not None:
            if old is None:
                del os.environ["HEYOKA_AMD_V5_OPTS"]
            else:
                os.environ["HEYOKA_AMD_V5_OPTS"] = old
    assert kernel in ta.hip_source_mode, ta.hip_source_mode
    if kernel == "v5":
        assert ("const hy_d2 w" in ta.hip_source) == (opts == "nofrx")  # (128-bit operand reads: only in the nofrx layout)
    return ta


@pytest.mark.parametrize("kernel", ["v5", "v5-nofrx", "v3", "v2"])
def test_emulated_cluster_kernels_single_step_vs_oracle(kernel):
    """One Taylor step of 11 perturbed outer Solar Systems (ragged: the last wavefront holds replicas) with the strict
    (no contraction) host build of the generated source: step sizes to 1e4 eps, states and Taylor coefficients to 1e5 eps
    of the oracle's - the tolerances of the GPU parity tests built with -ffp-contract=off."""
    n = 11
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    ta = _outer_ss(kernel)
    k = emu.EmulatedKernel(ta.hip_source)
    r = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=36 * (ta.order + 1))
    ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True)
    ora.step(wtc=True)
    h_o = np.array([h for _, h in ora.step_res])
    assert rel_err(r["last_h"], h_o) <= 1e4 * EPS
    assert rel_err(r["state"], ora.state.reshape(36, n)) <= 1e5 * EPS
    assert rel_err(r["time_hi"], ora.time_hi) <= 1e4 * EPS
    tc_o = ora.tc.reshape(36, ta.order + 1, n)
    scale = np.max(np.abs(tc_o), axis=2, keepdims=True) + 1e-300
    assert np.max(np.abs(r["tc"].reshape(tc_o.shape) - tc_o) / scale) <= 1e5 * EPS


def test_emulated_v5_propagation_through_the_work_queue_with_refill():
    """propagate_until() of 37 systems with per-system final times through ONE workgroup (32 systems in flight): the
    device-side queue, the retire / refill path of the one-lane-per-pair kernel and the frozen bookkeeping of finished
    systems, lane by lane against the oracle's ensemble driver."""
    n = 37
    rng = np.random.RandomState(3)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=77)
    tf = 4.0 * rng.uniform(0.2, 1.5, n)
    ta = _outer_ss("v5")
    k = emu.EmulatedKernel(ta.hip_source)
    r = k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=tf, max_grid=1)
    ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True)
    ora.propagate_until(tf)
    assert np.array_equal(r["outcome"], np.array([int(p[0]) for p in ora.prop_res]))
    assert np.array_equal(r["time_hi"], tf)
    ns_o = np.array([int(p[3]) for p in ora.prop_res])
    assert np.abs(r["n_steps"].astype(np.int64) - ns_o).max() <= 1
    assert rel_err(r["state"], ora.state.reshape(36, n)) <= 1e5 * EPS


def test_emulated_v5_taylor_coefficients_by_threshold():
    """Single-step launch with hy_kargs::pad bit 2 (the lock-step loop of propagate_grid() without a callback): a.tfin_hi holds a
    time per system, and only the systems whose step reaches it store their Taylor coefficients - bit for bit the
    coefficients of the launch which stores them all; state, step sizes and times do not depend on it."""
    n = 11
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    ta = _outer_ss("v5")
    k = emu.EmulatedKernel(ta.hip_source)
    rows = 36 * (ta.order + 1)
    full = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows)
    thr = np.where(np.arange(n) % 2 == 0, 0.01, 1e9)  # (a step of the outer Solar System is ~0.4 yr)
    part = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows, tfin=thr, pad=4)
    for key in ("state", "last_h", "time_hi", "time_lo"):
        assert np.array_equal(full[key], part[key]), key
    reached = full["time_hi"] >= thr
    assert reached.any() and not reached.all()
    assert np.array_equal(part["tc"][:, reached], full["tc"][:, reached])
    assert np.all(part["tc"][:, ~reached] == 0.0)
    # Backward in time: the comparison turns around.
    fullb = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, -np.inf), want_tc_rows=rows)
    partb = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, -np.inf), want_tc_rows=rows, tfin=-thr, pad=4)
    assert np.array_equal(partb["tc"][:, reached], fullb["tc"][:, reached])
    assert np.all(partb["tc"][:, ~reached] == 0.0)
    # The LAST step of a lane is clamped to the remaining time rem.hi and ends at tlast - rem.lo: with a grid ending at 0
    # (or crossing 0) the high part of the new time lands on either side of the last grid time, while hy_grid_post treats
    # the lane as done (h == rem.hi) and evaluates every remaining grid point from these coefficients - a clamped step
    # always stores (round-5 advisor finding: t = (-0.05, -+3e-18), limit 0.05, last grid time 0).
    for lo in (-3e-18, 3e-18):
        t_hi, t_lo = np.full(n, -0.05), np.full(n, lo)
        fullc = k.run(st, t_hi, t_lo, mode=0, lim=np.full(n, 0.05), want_tc_rows=rows)
        partc = k.run(st, t_hi, t_lo, mode=0, lim=np.full(n, 0.05), want_tc_rows=rows, tfin=np.zeros(n), pad=4)
        assert np.all(fullc["last_h"] == 0.05)
        assert np.all(np.sign(fullc["time_hi"]) == np.sign(lo))  # (the new time is -+3e-18: both sides of the grid time)
        assert np.array_equal(partc["tc"], fullc["tc"]), lo


@pytest.mark.parametrize("nb,masses", [(3, None), (4, None), (3, [1.0, 1e-3, 3e-4]), (5, None), (6, None), (6, [3.0, 1e-3, 0.7, 2.0, 4e-3, 0.5]), (6, "default"),
                                       (6, [1.0, 1e-3, 1.0, 2.0, 1e-3, 0.5]), (7, "default"), (9, "default")])
def test_emulated_v5_other_systems_single_step_vs_oracle(nb, masses):
    """The one-lane-per-pair kernel with the reactions fused into the sums on other pair-interaction systems: 5 bodies (10
    pairs on 16 lanes, 15 sums: ONE glue round; 3 and 4 bodies - round 6: 3 pairs on 8 lanes, 6 pairs on 16, more lanes per
    system than pairs so that the jets of the systems of a CU fit in its LDS) and 6 bodies with other mass ratios than the outer Solar System's (comparable
    masses: reaction coefficients of order one). (Equal masses take model::nbody() to its grouped branch, whose clusters
    have another shape: those systems run on the lane-pair / first-generation kernels.)"""
    rng = np.random.RandomState(40 + nb)
    if masses is None:
        masses = list(1.0 / (1.0 + np.arange(nb)) ** 2)
    kw_g = {} if masses == "default" else {"masses": masses}
    n = 13
    pos = rng.uniform(-3.0, 3.0, (nb, 3, n)) + 6.0 * np.arange(nb)[:, None, None] * np.array([1.0, 0.3, -0.2])[None, :, None]
    vel = rng.uniform(-0.3, 0.3, (nb, 3, n))
    st = np.concatenate([np.concatenate([pos[b], vel[b]], axis=0) for b in range(nb)], axis=0)
    ta = hy.taylor_adaptive_batch(hy.model.nbody(nb, **kw_g), None, 64, high_accuracy=True, cluster_kernel="v5")
    assert "v5" in ta.hip_source_mode, ta.hip_source_mode
    assert "frc" in ta.hip_source  # (coefficient registers of the fused sums)
    k = emu.EmulatedKernel(ta.hip_source)
    rows = 6 * nb * (ta.order + 1)
    r = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows)
    ora = ho.OracleIntegrator(ho.nbody(nb, **kw_g), st, n, high_accuracy=True)
    ora.step(wtc=True)
    h_o = np.array([h for _, h in ora.step_res])
    assert rel_err(r["last_h"], h_o) <= 1e4 * EPS
    assert rel_err(r["state"], ora.state.reshape(6 * nb, n)) <= 1e5 * EPS
    tc_o = ora.tc.reshape(6 * nb, ta.order + 1, n)
    scale = np.max(np.abs(tc_o), axis=2, keepdims=True) + 1e-300
    assert np.max(np.abs(r["tc"].reshape(tc_o.shape) - tc_o) / scale) <= 1e5 * EPS


def test_emulated_multi_class_cluster_stepper_and_staged_table_stepper_vs_oracle():
    """Round 6. (a) A system whose clusters come in two shapes - a chain of pendula with cubic bonds: 16 sin / cos pairs of
    state variables, 15 cubes (as products) of differences - on the multi-class wave-cluster stepper (one section of code per class of
    clusters): built without contraction it keeps the reference's operation order, the Taylor coefficients of one step are
    the default-mode oracle's BIT FOR BIT. (b) The staged table stepper (tape in LDS, lanes
    over the nodes of a group) on the outer Solar System: with the strict order of the additions (kw::compact_mode) the
    COMPACT-mode oracle's coefficients bit for bit, with the terms of the convolutions dealt to several lanes 1e5 eps; a
    propagation through the device-side queue against the oracle."""
    from heyoka_amd import mixed_models as mm

    n, ns = 9, 16
    st = mm.sine_lattice_state(ns, n)
    ta = hy.taylor_adaptive_batch(mm.sine_lattice(hy, ns), None, 64)
    assert "2 classes of clusters" in ta.hip_source_mode, ta.hip_source_mode
    p = ta.order
    k = emu.EmulatedKernel(ta.hip_source)
    r = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=2 * ns * (p + 1),
              scratch_per_wave=(p + 1) * 4 * 64)
    ora = ho.OracleIntegrator(mm.sine_lattice(ho, ns), st, n)
    ora.step(wtc=True)
    # (The Taylor coefficients bit for bit; the step size goes through exp(log()) in the kernel and pow() in the oracle: a few
    # ulps, and the new state with it.)
    assert np.array_equal(r["tc"].reshape(2 * ns, p + 1, n), ora.tc.reshape(2 * ns, p + 1, n))
    assert rel_err(r["last_h"], np.array([h for _, h in ora.step_res])) <= 16 * EPS
    assert rel_err(r["state"], ora.state.reshape(2 * ns, n)) <= 1e3 * EPS

    n = 7
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    for compact in (True, False):
        ta = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), None, 64, high_accuracy=True, compact_mode=compact,
                                      emitter="table")
        assert "table mode (staged)" in ta.hip_source_mode and ("strict order" in ta.hip_source_mode) == compact
        k = emu.EmulatedKernel(ta.hip_source)
        r = k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=36 * 21)
        ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True, compact_mode=True)
        ora.step(wtc=True)
        tc_o = ora.tc.reshape(36, 21, n)
        if compact:
            assert np.array_equal(r["tc"].reshape(tc_o.shape), tc_o)
        else:
            scale = np.max(np.abs(tc_o), axis=2, keepdims=True) + 1e-300
            assert np.max(np.abs(r["tc"].reshape(tc_o.shape) - tc_o) / scale) <= 1e5 * EPS
        tf = np.linspace(1.0, 3.0, n)
        r = k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=tf, max_grid=2)
        ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True, compact_mode=True)
        ora.propagate_until(tf)
        assert np.array_equal(r["outcome"], np.array([int(q[0]) for q in ora.prop_res]))
        assert np.array_equal(r["n_steps"].astype(np.int64), np.array([int(q[3]) for q in ora.prop_res]))
        assert np.array_equal(r["time_hi"], tf)
        assert rel_err(r["state"], ora.state.reshape(36, n)) <= 1e5 * EPS


def test_emulated_v5_propagation_from_grid_point_to_grid_point():
    """Round 6: propagate-mode launches with hy_kargs::pad bit 2 (emitted_module::grid_multi_step) - the lock-step loop of
    propagate_grid() without a callback takes every system from one grid point to the next in ONE launch: the system leaves
    the step loop after the first step which reaches a.tc_thr[s] (not clamped there: only the last grid time a.tfin clamps),
    with the Taylor coefficients of THAT step stored. Checked: the exit step brackets the threshold, counters and outcomes,
    and the dense output of the stored coefficients at the threshold against the oracle propagated to that time; through the
    retire / refill path of the work queue (37 systems on one workgroup) with per-system thresholds."""
    n = 37
    rng = np.random.RandomState(11)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=21)
    thr = rng.uniform(0.3, 2.5, n)
    ta = _outer_ss("v5")
    k = emu.EmulatedKernel(ta.hip_source)
    p = ta.order
    r = k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=np.full(n, 100.0), pad=4, tc_thr=thr, want_tc_rows=36 * (p + 1), max_grid=1)
    t1, h = r["time_hi"], r["last_h"]
    assert np.all(r["outcome"] == int(hy.taylor_outcome.success))
    assert np.all(t1 >= thr) and np.all(t1 - h < thr)  # the exit step is the first one which reaches the threshold
    assert np.all(r["n_steps"] >= 1) and np.all(r["n_steps"] == np.ceil(np.round(r["n_steps"])))
    # Dense output at the threshold from the stored coefficients (Horner in extended precision is not needed at 1e-13).
    tc = r["tc"].reshape(36, p + 1, n)
    hd = thr - (t1 - h)
    dense = np.zeros((36, n))
    for kk in range(p, -1, -1):
        dense = dense * hd + tc[:, kk, :]
    ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True)
    ora.propagate_until(thr)
    ref = ora.state.reshape(36, n)
    assert np.max(np.abs(dense - ref) / (np.max(np.abs(ref), axis=1, keepdims=True))) <= 1e5 * EPS
    # The clamp at the last grid time still holds: a threshold beyond it ends with time_limit exactly there.
    r2 = k.run(st[:, :4], np.zeros(4), np.zeros(4), mode=1, tfin=np.full(4, 1.0), pad=4, tc_thr=np.full(4, np.inf), want_tc_rows=36 * (p + 1))
    assert np.all(r2["time_hi"] == 1.0) and np.all(r2["outcome"] == int(hy.taylor_outcome.time_limit))
    # hy_kargs::grid_done: 1 for the systems whose last step was clamped to the remaining time, 0 for a grid-point exit.
    assert np.all(r2["grid_done"] == 1.0) and np.all(r["grid_done"] == 0.0)


def test_emulated_v5_grid_launch_with_a_lane_which_goes_nonfinite():
    """The multi-step grid launch (hy_kargs::pad bit 2, a.tc_thr) with a system which goes non-finite between two grid points
    (Jupiter falling radially onto the Sun, t = 0.597): that system ends with err_nf_state and the counters of the steps
    BEFORE the non-finite one - its own lock-step propagation in the oracle (hy_grid_post adds them with per-lane semantics;
    with the reference's semantics the host rolls the launch back, counters[0] says so) - while the others run on to the
    grid point."""
    n = 5
    st = configs.outer_ss_state(n, perturb=1e-6, seed=3).reshape(36, n).copy()
    st[6:9, 1] = st[0:3, 1] + np.array([2.25, 0.0, 0.0])
    st[9:12, 1] = st[3:6, 1]
    ta = _outer_ss("v5")
    k = emu.EmulatedKernel(ta.hip_source)
    p = ta.order
    r = k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=np.full(n, 4.0), lim=np.full(n, 0.01), pad=4, tc_thr=np.full(n, 1.0),
              want_tc_rows=36 * (p + 1), max_grid=1)
    assert r["counters"][0] == 1
    assert r["outcome"][1] == int(hy.taylor_outcome.err_nf_state)
    ok = [0, 2, 3, 4]
    assert np.all(r["time_hi"][ok] >= 1.0) and np.all(r["time_hi"][ok] - r["last_h"][ok] < 1.0)
    solo = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st[:, 1:2], 1, high_accuracy=True)
    (oc, mn, mx, ns), = solo.propagate_until(4.0, max_delta_t=0.01)
    assert oc == ho.OC_ERR_NF_STATE
    print("[emulated v5, diverging system] steps %d (oracle %d), min |h| %.17g (oracle %.17g), max |h| %.17g (oracle %.17g)"
          % (int(r["n_steps"][1]), ns, r["min_h"][1], mn, r["max_h"][1], mx))
    assert int(r["n_steps"][1]) == ns
    assert abs(r["max_h"][1] - mx) <= 1e-9 * mx and abs(r["min_h"][1] - mn) <= 1e-9 * mn


# ---- batch-size independence (the CPU half of tests/test_batch_independence.py) ----
def _independence_kernels():
    from heyoka_amd import mixed_models as mm

    def outer(kernel, **kw):
        return lambda: (_outer_ss(kernel, **kw), lambda n: configs.outer_ss_state(n, perturb=1e-3, seed=9), {})

    def cloud(nb):
        def state(n):
            rng = np.random.RandomState(40 + nb)
            pos = rng.uniform(-3.0, 3.0, (nb, 3, n)) + 6.0 * np.arange(nb)[:, None, None] * np.array([1.0, 0.3, -0.2])[None, :, None]
            vel = rng.uniform(-0.3, 0.3, (nb, 3, n))
            return np.concatenate([np.concatenate([pos[b], vel[b]], axis=0) for b in range(nb)], axis=0)

        masses = list(1.0 / (1.0 + np.arange(nb)) ** 2)
        return lambda: (hy.taylor_adaptive_batch(hy.model.nbody(nb, masses=masses), None, 64, high_accuracy=True, cluster_kernel="v5"), state, {})

    def lattice():
        ta = hy.taylor_adaptive_batch(mm.sine_lattice(hy, 16), None, 64)
        return ta, lambda n: mm.sine_lattice_state(16, n), {"scratch_per_wave": (ta.order + 1) * 4 * 64}

    def staged():
        ta = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), None, 64, high_accuracy=True, emitter="table")
        return ta, lambda n: configs.outer_ss_state(n, perturb=1e-3, seed=9), {}

    # name: (builder of (integrator, states, extra launch arguments), expected mode, systems per wavefront / workgroup,
    # horizon of the propagation through the work queue or None)
    return {
        "v5": (outer("v5"), "mode v5", 4, 2.0), "v5-nofrx": (outer("v5-nofrx"), "mode v5", 4, 2.0),
        "v3": (outer("v3"), "mode v3", 2, None), "v2": (outer("v2"), "mode v2", 4, None),
        "v5-nbody3": (cloud(3), "mode v5", 8, 6.0), "v5-nbody4": (cloud(4), "mode v5", 4, 6.0), "v5-nbody8": (cloud(8), "mode v5", 2, 6.0),
        "multi-class": (lattice, "2 classes of clusters", 4, None), "staged": (staged, "table mode (staged)", 1, None),
    }


@pytest.mark.parametrize("name", sorted(_independence_kernels()))
def test_emulated_kernels_results_do_not_depend_on_the_batch_size(name):
    """The integration of a system depends on nothing but that system: one step with all Taylor coefficients of 1, 2, 3,
    S - 1, S and S + 1 systems (S: the systems of a wavefront, or of a workgroup for the staged stepper) and of a window
    of a larger batch gives BIT FOR BIT the columns of the run of that larger batch (2 S + 3 systems): states, times, step
    sizes, outcomes and every Taylor coefficient. For the one-lane-per-pair kernel also a propagation with per-system
    final times through the work queue of ONE workgroup, the larger batch 5 systems beyond what the workgroup keeps in
    flight (as test_emulated_v5_propagation_through_the_work_queue_with_refill: 37 systems on 32 slots), so that systems
    which were REFILLED into the lanes of a finished system are compared with their own first-fill runs - counters and
    smallest / largest steps included. One compilation per kernel. The GPU half - every family, the
    propagation loops, the grid, events - is tests/test_batch_independence.py; a difference there which this test does not
    show is the hardware's side of the packing (cross-lane operations with idle lanes, LDS slabs of absent systems, launch
    geometry), not the generators' arithmetic."""
    from test_batch_independence import systems_per_unit

    build, want, S_expected, horizon = _independence_kernels()[name]
    ta, state, extra = build()
    assert want in ta.hip_source_mode, ta.hip_source_mode
    S = systems_per_unit(ta.hip_source_mode)
    assert S == S_expected, ta.hip_source_mode
    k = emu.EmulatedKernel(ta.hip_source)
    sizes = sorted({1, 2, 3, S - 1, S, S + 1} - {0})
    window = np.arange(3, 3 + S + 1)
    n_big = max(2 * S + 3, 5)
    st = state(n_big)
    rows = st.shape[0] * (ta.order + 1)
    big = k.run(st, np.zeros(n_big), np.zeros(n_big), mode=0, lim=np.full(n_big, np.inf), want_tc_rows=rows, **extra)
    assert np.all(big["last_h"] > 0) and np.isfinite(big["tc"]).all()
    for idx in [np.arange(n) for n in sizes] + [window]:
        n = len(idx)
        part = k.run(st[:, idx], np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows, **extra)
        for key in ("state", "time_hi", "time_lo", "last_h", "outcome", "tc"):
            assert np.array_equal(part[key], big[key][..., idx]), (name, "step", key, "systems %d .. %d" % (idx[0], idx[-1]))
    if horizon is None:
        return
    # The propagation: ONE workgroup keeps `slots` systems in flight, the larger run holds 5 more - the systems slots ..
    # slots + 4 are pulled from the queue by the lanes of systems which have finished and inherit their registers and
    # bookkeeping slabs (the retire / refill path). The small prefixes and the window slots - 2 .. slots + 4 on their own
    # are all first-fill systems: refilled and first-fill runs of the same system are compared bit for bit.
    assert "snew < N" in ta.hip_source  # (this kernel has the refill path)
    slots = k.block // k.lanes_per_system
    n_prop = slots + 5
    st = state(n_prop)
    tf = horizon * np.random.RandomState(1).uniform(0.5, 1.5, n_prop)
    bigp = k.run(st, np.zeros(n_prop), np.zeros(n_prop), mode=1, tfin=tf, max_grid=1, **extra)
    assert np.array_equal(bigp["time_hi"], tf) and np.unique(bigp["n_steps"]).size > 1
    for idx in [np.arange(n) for n in sizes] + [window, np.arange(slots - 2, n_prop)]:
        n = len(idx)
        part = k.run(st[:, idx], np.zeros(n), np.zeros(n), mode=1, tfin=tf[idx], max_grid=1, **extra)
        for key in ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "min_h", "max_h"):
            assert np.array_equal(part[key], bigp[key][..., idx]), (name, "propagation", key, "systems %d .. %d" % (idx[0], idx[-1]))


def test_batch_independence_families_select_their_kernels():
    """Every family of tests/test_batch_independence.py reaches the kernel it names (no GPU is needed to generate the
    source), the source of a family is the same for every batch size, and S - the systems which one wavefront or
    workgroup serves, as the GPU test derives it from hip_source_mode - is what DESIGN.md tabulates."""
    import test_batch_independence as tbi

    S_table = {"v5": 4, "v5_32_lanes": 2, "v5_8_lanes_lds_jets": 8, "v5_16_lanes_lds_jets": 4, "v5_events": 4, "v3": 2, "v3_64_lanes": 1,
               "v2": 4, "v2_aliased": 4, "multi_class": 4, "unrolled": 64, "unrolled_two_waves": 64, "unrolled_register_jets": 64,
               "staged": 1, "table_hbm": 64, "staged_functions": 1, "table_hbm_functions": 64, "block_centres": 1, "block_v2": 1,
               "block_v2_nbody64": 1}
    assert set(S_table) == set(tbi.FAMILIES)
    assert tbi.sizes_for(4, 131) == [1, 2, 3, 4, 5, 9, 65] and tbi.sizes_for(1, 131) == [1, 2, 3, 65]
    assert tbi.sizes_for(64, 131) == [1, 2, 3, 63, 64, 65, 129] and tbi.sizes_for(8, 131) == [1, 2, 3, 7, 8, 9, 17, 65]
    assert tbi.sizes_for(2, 131) == [1, 2, 3, 5, 65]
    for name, fam in tbi.FAMILIES.items():
        kw = dict(fam.get("kw", {}))
        src = set()
        for n in (1, 3, tbi.N_POOL):
            if fam.get("events"):
                kw.update(tbi._outer_ss_events(hy, []))
            with tbi._env(fam.get("env")):
                ta = hy.taylor_adaptive_batch(fam["sys"](hy), None, n, **kw)
            for w in fam["want"]:
                assert w in ta.hip_source_mode, (name, w, ta.hip_source_mode)
            assert fam.get("not_want", "\0") not in ta.hip_source_mode, (name, ta.hip_source_mode)
            assert tbi.systems_per_unit(ta.hip_source_mode) == S_table[name], (name, ta.hip_source_mode)
            src.add(ta.hip_source)
        assert len(src) == 1, name + ": the generated source depends on the batch size"
