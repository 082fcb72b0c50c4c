"""The LDS-side items of the one-lane-per-pair stepper ("v5") change WHICH instruction is issued WHEN, never an
operation or its order: the kernel with the jet reads of the final evaluation issued ahead of the selector's log / exp
chain must give bit for bit the results of the kernel with the item switched off (HEYOKA_AMD_V5_OPTS=notailrd: the reads
behind the step size, where the series consume them). The exec-masked variants of the second glue round, of the replica
lane and of the partially filled pass were rejected by the microbenchmark (profiles/HISTORY.md: an LDS instruction costs
the same whatever its EXEC mask), the operand reads of a round ahead of the chains of the round before by their A/B; they
do not exist, so "notailrd" is every new flag. CPU: the generated source compiled for the host under the wavefront
emulator of tests/emu; -m gpu: the same comparisons through the C ABI on 4 096 systems and on one launch of the
benchmark's size."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import codegen_check, configs  # noqa: E402

M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
OFF = "notailrd"  # (every new switch-off flag of HEYOKA_AMD_V5_OPTS)
TAIL_MARKER = "Jet reads of the final evaluation issued ahead of the selector"


def _cloud_state(nb, n):
    rng = np.random.RandomState(40 + nb)
    pos = rng.uniform(-3.0, 3.0, (nb, 3, n)) + 6.0 * np.arange(nb)[:, None, None] * np.array([1.0, 0.3, -0.2])[None, :, None]
    vel = rng.uniform(-0.3, 0.3, (nb, 3, n))
    return np.concatenate([np.concatenate([pos[b], vel[b]], axis=0) for b in range(nb)], axis=0)


# name: (bodies, lanes per system, horizon of the propagation): 16 lanes (the headline), the 32- and 64-lane variants, and
# the 8- and 16-lane variants of the few-pair systems. All of them take the new placement (asserted).
VARIANTS = {
    "outer_ss_16_lanes": (6, 16, 2.0),
    "nbody8_32_lanes": (8, 32, 6.0),
    "nbody10_64_lanes": (10, 64, 6.0),
    "nbody3_8_lanes": (3, 8, 6.0),
    "nbody4_16_lanes": (4, 16, 6.0),
}


def _build(nb, opts, st=None, n=64, **kw):
    old = os.environ.get("HEYOKA_AMD_V5_OPTS")
    if opts:
        os.environ["HEYOKA_AMD_V5_OPTS"] = opts
    else:
        os.environ.pop("HEYOKA_AMD_V5_OPTS", None)
    try:
        if nb == 6:
            sys_ = hy.model.nbody(6, masses=M, Gconst=G)
        else:
            sys_ = hy.model.nbody(nb, masses=list(1.0 / (1.0 + np.arange(nb)) ** 2))
        ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, cluster_kernel="v5", **kw)
    finally:
        if old is None:
            os.environ.pop("HEYOKA_AMD_V5_OPTS", None)
        else:
            os.environ["HEYOKA_AMD_V5_OPTS"] = old
    assert "mode v5" in ta.hip_source_mode, ta.hip_source_mode
    return ta


def _state(nb, n, perturb=1e-3):
    return configs.outer_ss_state(n, perturb=perturb, seed=9) if nb == 6 else _cloud_state(nb, n)


def _check_layout(new, off, lanes):
    """The variant takes the new placement, visibly: the marker and another text in the tail, the same text in the orders."""
    assert "lanes per system: %d," % lanes in new.hip_source_mode, new.hip_source_mode
    assert TAIL_MARKER in new.hip_source and TAIL_MARKER not in off.hip_source and new.hip_source != off.hip_source
    body = lambda t: t[t.index("double m0 = 0.0, mo = 0.0, mom1 = 0.0;"):t.index("m0 = hy_nmax(m0, hy_dpp")]
    assert body(new.hip_source) == body(off.hip_source)
    # (Every read issued ahead of the selector is the one its series consumes: each name defined once and used once.)
    names = re.findall(r"const double (trd\d+) = ", new.hip_source)
    assert len(names) >= 20 and len(set(names)) == len(names) and "trd" not in off.hip_source
    for nm in names:
        assert len(re.findall(r"\b%s\b" % nm, new.hip_source)) == 2, nm
    # (EXEC is never touched by hand: the exec-masked LDS rounds were not built.)
    assert "s_mov_b64 exec" not in new.hip_source and "saveexec" not in new.hip_source


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_emulated_tail_read_placement_is_bit_identical_to_the_kernel_without_it(name):
    """One step with all Taylor coefficients of 11 systems, and propagate_until() with per-system final times of 5 systems
    more than ONE workgroup keeps in flight (37 for 16 lanes per system: the retire / refill path), default kernel against
    the kernel with every new flag off: state, times, last_h, coefficients, step counts, outcomes, extreme steps."""
    import emu

    nb, lanes, horizon = VARIANTS[name]
    new, off = _build(nb, ""), _build(nb, OFF)
    _check_layout(new, off, lanes)
    kn, ko = emu.EmulatedKernel(new.hip_source), emu.EmulatedKernel(off.hip_source)
    n = 11
    st = _state(nb, n)
    rows = st.shape[0] * (new.order + 1)
    rn, ro = [k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows) for k in (kn, ko)]
    assert np.all(rn["last_h"] > 0) and np.isfinite(rn["tc"]).all() and np.any(rn["tc"][-1] != 0.0)
    for key in ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "tc"):
        assert np.array_equal(rn[key], ro[key]), (name, "step", key)
    # (The refill path: per system wherever a wavefront holds several systems; a 64-lane system has its wavefront to itself.)
    assert ("snew < N" in new.hip_source) == (lanes < 64)
    n = kn.block // kn.lanes_per_system + 5
    st = _state(nb, n)
    tf = horizon * np.random.RandomState(1).uniform(0.5, 1.5, n)
    pn, po = [k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=tf, max_grid=1) for k in (kn, ko)]
    assert np.array_equal(pn["time_hi"], tf) and np.unique(pn["n_steps"]).size > 1
    for key in ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "min_h", "max_h"):
        assert np.array_equal(pn[key], po[key]), (name, "propagation", key)


def test_the_stepper_with_events_keeps_its_layout():
    """The stepper with events stays on the nofrx layout and takes no final step in the kernel's tail: the same text with
    and without the new flags."""
    x1, x2 = hy.make_vars("x_1", "x_2")
    src = []
    for opts in ("", OFF):
        ta = _build(6, opts, nt_events=[hy.nt_event((x1 - x2) * (x1 - x2) - 4.0, lambda *a: None)])
        assert "events:" in ta.hip_source_mode, ta.hip_source_mode
        assert TAIL_MARKER not in ta.hip_source
        src.append(ta.hip_source)
    assert src[0] == src[1]


def test_kernel_resources_with_the_tail_read_placement():
    """256 registers, two wavefronts per SIMD, no more spilled dwords than the 18 of the kernel before the change, LDS
    within 160 KB; the other lane variants spill no more than without the placement."""
    res = codegen_check.kernel_resources(_build(6, "").code_object)
    assert res["vgpr_total"] == 256 and res["waves_per_simd_by_registers"] == 2, res
    assert res["vgpr_spill"] <= 18 and res["lds_bytes"] <= 160 * 1024, res
    for nb in (3, 4, 8, 10):
        new, off = [codegen_check.kernel_resources(_build(nb, o).code_object) for o in ("", OFF)]
        assert new["vgpr_spill"] <= off["vgpr_spill"] and new["vgpr_total"] <= 256, (nb, new, off)


def _gpu_outputs(ta, prop, tc_on_host=True):
    out = {"state": ta.state, "time_hi": ta.dtime[0], "time_lo": ta.dtime[1], "last_h": ta.last_h}
    if prop:
        oc, mn, mx, ns = ta.propagate_res_arrays()
        out.update(outcome=np.asarray(oc), min_h=np.asarray(mn), max_h=np.asarray(mx), n_steps=np.asarray(ns))
    else:
        out.update(outcome=np.array([int(oc) for oc, _ in ta.step_res]))
        if tc_on_host:
            out.update(tc=ta.tc)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 1048576], ids=["4096_systems", "full_size_launch"])
def test_gpu_tail_read_placement_is_bit_identical_and_deterministic(n):
    """On the GPU, 4 096 systems and one launch of the benchmark's size: one step with all Taylor coefficients (the 6 GB of
    coefficients of 2^20 systems are compared where they are, in device memory) and a propagate_until() with per-system
    final times, default kernel against the kernel with every new flag off, and the default kernel twice on fresh
    integrators: all outputs array_equal."""
    import torch

    small = n == 4096
    st = configs.outer_ss_state(n, perturb=1e-3 if small else 1e-12, seed=42)
    tf = 30.0 * np.random.RandomState(1).uniform(0.5, 1.5, n)
    new, off, again = _build(6, "", st, n), _build(6, OFF, st, n), _build(6, "", st, n)
    _check_layout(new, off, 16)
    assert again.hip_source == new.hip_source
    outs = []
    for ta in (new, off):
        ta.step(write_tc=True)
        outs.append(_gpu_outputs(ta, False, tc_on_host=small))
    assert np.all(outs[0]["last_h"] > 0) and np.all(outs[0]["outcome"] == outs[0]["outcome"][0])
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key]), ("step", key)
    tcs = [torch.as_tensor(ta.device_array("tc"), device="cuda") for ta in (new, off)]
    assert bool(torch.isfinite(tcs[0]).all()) and bool((tcs[0][-1, -1] != 0).any())
    assert torch.equal(tcs[0], tcs[1])
    del tcs
    # (The second run of the default kernel takes the same first step, without the coefficients.)
    again.step()
    assert np.array_equal(again.state, new.state) and np.array_equal(again.last_h, new.last_h)
    res = []
    for ta in (new, off, again):
        ta.propagate_until(tf)
        res.append(_gpu_outputs(ta, True))
    assert np.array_equal(res[0]["time_hi"], tf) and np.unique(res[0]["n_steps"]).size > 1
    for key in res[0]:
        assert np.array_equal(res[0][key], res[1][key]), ("propagation, flags off", key)
        assert np.array_equal(res[0][key], res[2][key]), ("propagation, second run", key)
