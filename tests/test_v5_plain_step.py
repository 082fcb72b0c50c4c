"""The plain step of the one-lane-per-pair stepper ("v5"): a wavefront none of whose systems is finished, clamped by the
remaining time or the maximum step, at its step limit or non-finite in this step leaves out the bookkeeping which decides
those things - behind one ballot it advances the time, the counters and the extreme steps and stores the state without
selects; the remaining time is no longer carried from step to step (a lower bound of its magnitude is, the ordinary path
recomputes the exact value). No arithmetic of a result changes, so the kernel must give bit for bit the results of the kernel
with the item switched off (HEYOKA_AMD_V5_OPTS=noplainstep, which restores the text of before). CPU: the generated source
under the wavefront emulator of tests/emu, every case the issue lists; -m gpu: the same comparisons on 4 099 and 40 003
systems.

One module serves step(), propagate_until() and the launches of propagate_grid() (hy_kargs::mode and ::pad are arguments
of the launch), so "the step kernel keeps its text" cannot be said of the source: those launches fail the scalar part of the
predicate (HY_PLAIN_STEP) and run the ordinary path - asserted on the text of that macro, and compared bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402
from test_v5_lane_sums import _build_default_masses  # noqa: E402
from test_v5_lds_diet import VARIANTS, _build, _gpu_outputs, _state  # noqa: E402

OFF = "noplainstep"
PHRASE = "plain steps leave out the bookkeeping of the step loop"
SCALAR = "#define HY_PLAIN_STEP ((HY_MODE == 1) & ((a.pad & 4) == 0) & (a.tc == nullptr))"
STEP_KEYS = ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "tc")
PROP_KEYS = ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "min_h", "max_h", "counters")
# (The step counter of the plain path in the emulated source: see _plain_counts().)
PLAIN_COUNT = "    n_steps = n_steps + 1u;\n    iter = iter + 1u;\n"
HORIZON = VARIANTS["outer_ss_16_lanes"][2]


def _check_takes_the_path(new, off):
    assert PHRASE in new.hip_source_mode and PHRASE not in off.hip_source_mode, (new.hip_source_mode, off.hip_source_mode)
    assert new.hip_source != off.hip_source
    # (Two wave-uniform branches on a ballot in plain C++ - in front of the final evaluation and behind it -, no hand-written
    # EXEC manipulation, no assembly for them; the remaining time is not carried.)
    assert new.hip_source.count(SCALAR) == 1 and new.hip_source.count("if (HY_PLAIN_STEP && __builtin_amdgcn_ballot_w64(pl_no") == 2
    assert "HY_PLAIN_STEP" not in off.hip_source and "rlb" not in off.hip_source
    assert "rem_new" not in new.hip_source and "rem_new" in off.hip_source
    assert new.hip_source.count(PLAIN_COUNT) == 1
    assert "s_mov_b64 exec" not in new.hip_source and "saveexec" not in new.hip_source
    assert new.hip_source.count("asm") == off.hip_source.count("asm")


_KERNELS = {}


def _headline():
    """(default integrator, flag-off integrator, their emulated kernels, the emulated default kernel whose plain path also
    counts its steps in the upper half of n_steps): built once, shared by the cases."""
    if not _KERNELS:
        import emu

        new, off = _build(6, ""), _build(6, OFF)
        _check_takes_the_path(new, off)
        counted = new.hip_source.replace(PLAIN_COUNT, PLAIN_COUNT.replace("1u;\n    iter", "1u + (1ull << 32);\n    iter"))
        _KERNELS.update(new=new, off=off, kn=emu.EmulatedKernel(new.hip_source), ko=emu.EmulatedKernel(off.hip_source),
                        kc=emu.EmulatedKernel(counted))
    return _KERNELS


def _plain_counts(st, **kw):
    """Per system: how many of its steps took the plain path (the same launch on the kernel which counts them)."""
    k = _headline()
    n = st.shape[1]
    t0 = kw.pop("t0", np.zeros(n))
    r = k["kc"].run(st, t0, np.zeros(n), mode=1, max_grid=1, **kw)
    return (r["n_steps"] >> np.uint64(32)).astype(np.int64), (r["n_steps"] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def _both(st, keys=PROP_KEYS, kernels=None, **kw):
    """The launch on the default and on the flag-off kernel, every output compared; the outputs of the default kernel."""
    k = kernels or (_headline()["kn"], _headline()["ko"])
    n = st.shape[1]
    t0 = kw.pop("t0", np.zeros(n))
    kw.setdefault("mode", 1)
    kw.setdefault("max_grid", 1)
    rn, ro = [x.run(st, t0, np.zeros(n), **kw) for x in k]
    for key in keys:
        # (Of the launch's counters the first is a result - the systems which met a non-finite state; the position of the work
        # queue depends on the order in which the emulator runs the wavefronts.)
        assert np.array_equal(rn[key][:1] if key == "counters" else rn[key], ro[key][:1] if key == "counters" else ro[key], equal_nan=True), key
    return rn


def _natural_step():
    """The largest step of the headline's systems as the selector chooses them (no limit), over a few steps: the first step
    of these initial conditions is a shorter one."""
    if "h_nat" not in _KERNELS:
        st = _state(6, 11)
        _KERNELS["h_nat"] = (st, _both(st, keys=("max_h",), tfin=np.full(11, 3.0))["max_h"])
    return _KERNELS["h_nat"]


def test_one_step_with_all_taylor_coefficients():
    """11 systems, mode 0, coefficients requested: the ordinary path (HY_PLAIN_STEP is false), bit for bit."""
    k = _headline()
    st = _state(6, 11)
    rows = st.shape[0] * (k["new"].order + 1)
    r = _both(st, keys=STEP_KEYS, mode=0, lim=np.full(11, np.inf), want_tc_rows=rows, max_grid=2)
    assert np.all(r["last_h"] > 0) and np.isfinite(r["tc"]).all() and np.any(r["tc"][-1] != 0.0)


def test_per_system_final_times_with_retire_and_refill():
    """Five systems more than one workgroup keeps in flight, final times T * U(0.5, 1.5): the systems of a wavefront leave the
    plain path at different steps and finished ones are replaced. Most steps are plain ones, never the first or the last of
    a system."""
    k = _headline()
    assert "snew < N" in k["new"].hip_source
    n = k["kn"].block // k["kn"].lanes_per_system + 5
    st = _state(6, n)
    tf = 3.0 * HORIZON * np.random.RandomState(1).uniform(0.5, 1.5, n)
    r = _both(st, tfin=tf)
    assert np.array_equal(r["time_hi"], tf) and np.unique(r["n_steps"]).size > 1 and r["counters"][0] == 0
    plain, total = _plain_counts(st, tfin=tf)
    print("plain steps per system:", plain, "of", total)
    assert np.array_equal(total, r["n_steps"].astype(np.int64))
    # (A step is plain for the four systems of a wavefront or for none, so a system's share depends on its neighbours.)
    assert np.all(plain <= np.maximum(total - 2, 0)) and 3 * plain.sum() > total.sum()


@pytest.mark.parametrize("factor", [0.5, 1.5, 2.0])
def test_max_delta_t_around_the_natural_step(factor):
    """max_delta_t below the natural step (every step clamped: no plain step), at 1.5 times it (no step clamped, but almost
    all of them inside the factor-2 margin of the predicate) and at twice it (steps on both sides of the margin). The counts
    of plain steps are printed."""
    st, h0 = _natural_step()
    n = st.shape[1]
    mdt = np.full(n, factor * np.median(h0))
    tf = np.full(n, 12.0 * np.median(h0))
    r = _both(st, tfin=tf, lim=mdt)
    assert np.array_equal(r["time_hi"], tf)
    plain, total = _plain_counts(st, tfin=tf, lim=mdt)
    print("factor", factor, "plain steps per system:", plain, "of", total, "max_h / mdt:", r["max_h"] / mdt)
    assert np.all(r["max_h"] <= mdt) and np.all(total >= 3)
    if factor < 1.0:
        assert plain.sum() == 0


def test_backward_in_time():
    st, h0 = _natural_step()
    n = st.shape[1]
    tf = -6.0 * np.median(h0) * np.random.RandomState(2).uniform(0.5, 1.5, n)
    r = _both(st, tfin=tf)
    assert np.array_equal(r["time_hi"], tf) and np.all(r["last_h"] < 0)
    plain, total = _plain_counts(st, tfin=tf)
    assert plain.sum() > 0 and np.all(plain <= np.maximum(total - 2, 0)), (plain, total)


def test_step_limit():
    """max_steps = 3: the third step of every system is an ordinary one and reports the step limit."""
    st, h0 = _natural_step()
    n = st.shape[1]
    tf = np.full(n, 20.0 * np.median(h0))
    r = _both(st, tfin=tf, max_steps=3)
    assert np.all(r["n_steps"] == 3) and np.all(r["outcome"] == r["outcome"][0]) and np.all(r["time_hi"] < tf)
    plain, total = _plain_counts(st, tfin=tf, max_steps=3)
    assert np.all(plain == 1) and np.all(total == 3), (plain, total)


def test_final_time_at_and_just_beyond_the_current_time():
    st = _state(6, 11)
    n = st.shape[1]
    t0 = np.full(n, 0.75)
    tf = t0 + np.where(np.arange(n) % 2 == 0, 0.0, 1e-3)
    r = _both(st, tfin=tf, t0=t0)
    assert np.array_equal(r["time_hi"], tf) and np.array_equal(r["n_steps"], (np.arange(n) % 2).astype(np.uint64))
    plain, _ = _plain_counts(st, tfin=tf, t0=t0)
    assert plain.sum() == 0


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_a_non_finite_system_next_to_finite_ones(bad):
    """A non-finite VALUE is ordinary data: the system ends with the non-finite outcome in its first step, is counted once,
    and its neighbours - the other systems of its wavefront among them - are what they are without it."""
    st, h0 = _natural_step()
    n = st.shape[1]
    tf = np.full(n, 5.0 * np.median(h0))
    clean = _both(st, tfin=tf)
    st2 = st.copy()
    st2[0, 5] = bad
    r = _both(st2, tfin=tf)
    ok = np.arange(n) != 5
    assert r["counters"][0] == 1 and clean["counters"][0] == 0
    assert r["outcome"][5] != clean["outcome"][5] and np.all(r["outcome"][ok] == clean["outcome"][ok])
    for key in ("state", "time_hi", "time_lo", "last_h", "n_steps", "min_h", "max_h"):
        assert np.array_equal(r[key][..., ok], clean[key][..., ok]), key


@pytest.mark.parametrize("name", sorted(set(VARIANTS) - {"outer_ss_16_lanes"}) + ["nbody6_default_masses"])
def test_every_variant_takes_the_path_bit_for_bit_or_keeps_its_text(name):
    """The other lane geometries of the generator and nbody(6) with default masses: which of them take the path is reported;
    one which does is compared bit for bit (one step, per-system final times), one which does not has the same source with
    and without the flag."""
    import emu

    if name == "nbody6_default_masses":
        new, off = _build_default_masses(""), _build_default_masses(OFF)
        nb, horizon = 6, 2.0
    else:
        nb, _, horizon = VARIANTS[name]
        new, off = _build(nb, ""), _build(nb, OFF)
    takes = PHRASE in new.hip_source_mode
    print("%s: %s" % (name, "plain steps" if takes else "declined, text unchanged"))
    if not takes:
        assert new.hip_source == off.hip_source
        return
    _check_takes_the_path(new, off)
    ks = (emu.EmulatedKernel(new.hip_source), emu.EmulatedKernel(off.hip_source))
    st = _state(nb, 11)
    r = _both(st, keys=STEP_KEYS, kernels=ks, mode=0, lim=np.full(11, np.inf), want_tc_rows=st.shape[0] * (new.order + 1), max_grid=2)
    assert np.all(r["last_h"] > 0) and np.isfinite(r["tc"]).all()
    n = ks[0].block // ks[0].lanes_per_system + 5
    tf = horizon * np.random.RandomState(1).uniform(0.5, 1.5, n)
    r = _both(_state(nb, n), kernels=ks, tfin=tf)
    assert np.array_equal(r["time_hi"], tf) and np.unique(r["n_steps"]).size > 1


def test_the_stepper_with_events_keeps_its_text():
    x1, x2 = hy.make_vars("x_1", "x_2")
    src = []
    for opts in ("", OFF):
        ta = _build(6, opts, nt_events=[hy.nt_event((x1 - x2) * (x1 - x2) - 4.0, lambda *a: None)])
        assert "events:" in ta.hip_source_mode and PHRASE not in ta.hip_source_mode, ta.hip_source_mode
        src.append(ta.hip_source)
    assert src[0] == src[1]


def test_the_other_generators_keep_their_text():
    """The lane-pair (v3, which kw::exact_division takes) and pipelined (v2) kernels."""
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    for kw in ({"cluster_kernel": "v3"}, {"cluster_kernel": "v2"}, {"exact_division": True}):
        src = []
        for opts in ("", OFF):
            old = os.environ.get("HEYOKA_AMD_V5_OPTS")
            os.environ["HEYOKA_AMD_V5_OPTS"] = opts
            try:
                ta = hy.taylor_adaptive_batch(sys_, None, 64, high_accuracy=True, **kw)
            finally:
                if old is None:
                    os.environ.pop("HEYOKA_AMD_V5_OPTS", None)
                else:
                    os.environ["HEYOKA_AMD_V5_OPTS"] = old
            assert PHRASE not in ta.hip_source_mode and "mode v5" not in ta.hip_source_mode, ta.hip_source_mode
            src.append(ta.hip_source)
        assert src[0] == src[1], kw


_STATIC_CHILD = r"""
import json, os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "profiles", "experiments")]
if sys.argv[3] == "torch":
    import torch
import isa_count
from heyoka_amd import codegen_check
from test_v5_lds_diet import _build
isa_count.OBJDUMP = codegen_check.find_objdump() or isa_count.OBJDUMP
new, off = _build(6, ""), _build(6, sys.argv[2])
print(json.dumps({"new": isa_count.step_loop_counts(new.code_object), "off": isa_count.step_loop_counts(off.code_object),
                  "res": codegen_check.kernel_resources(new.code_object), "res_off": codegen_check.kernel_resources(off.code_object),
                  "hazards": codegen_check.scan_code_object(new.code_object)}))
"""


@pytest.mark.parametrize("compiler", ["rocm", "torch"])
def test_kernel_resources_with_both_compilers(compiler):
    """Both kernels compiled for gfx950 in a process of their own - with ROCm's hiprtc, and with the one a process gets which
    has imported torch first (profiles/HISTORY.md, "Two compilers"): 256 registers, two wavefronts per SIMD, and no more
    spilled dwords than the flag-off kernel (the parent's text) built next to it. The static counts of the step loop hold both
    paths now and stand for no executed instruction: printed, not asserted."""
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k != "HEYOKA_AMD_V5_OPTS"}
    out = subprocess.run([sys.executable, "-c", _STATIC_CHILD, root, OFF, compiler], env=env, capture_output=True, text=True, check=True).stdout
    d = json.loads(out.strip().split("\n")[-1])
    print("step loop, new:", d["new"], "\nstep loop, off:", d["off"], "\nresources, new:", d["res"], "\nresources, off:", d["res_off"])
    res, res_off = d["res"], d["res_off"]
    assert res["vgpr_total"] == 256 and res["waves_per_simd_by_registers"] == 2, res
    assert res["vgpr_spill"] <= res_off["vgpr_spill"], (res, res_off)
    assert res["lds_bytes"] <= res_off["lds_bytes"] and d["hazards"] == [], d


def _gpu_case(st, n, prop, **kw):
    """default, flag off, default again on a fresh integrator: every output array_equal. Returns the first's outputs."""
    new, off, again = _build(6, "", st, n), _build(6, OFF, st, n), _build(6, "", st, n)
    _check_takes_the_path(new, off)
    assert again.hip_source == new.hip_source
    outs = []
    for ta in (new, off, again):
        prop(ta)
        outs.append(_gpu_outputs(ta, True))
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key], equal_nan=True), ("flag off", key)
        assert np.array_equal(outs[0][key], outs[2][key], equal_nan=True), ("second run", key)
    return outs[0]


_GPU_N = 4099  # (ragged: no multiple of the 4 systems of a wavefront or of the 32 of a workgroup)


def _gpu_natural_step(st):
    ta = _build(6, "", st, _GPU_N)
    ta.step()
    return float(np.median(ta.last_h))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["per_system_final_times", "max_delta_t_below", "max_delta_t_straddles", "backward", "non_finite_system"])
def test_gpu_plain_step_is_bit_identical_and_deterministic(case):
    n = _GPU_N
    st = configs.outer_ss_state(n, perturb=1e-3, seed=42)
    tf = 30.0 * np.random.RandomState(1).uniform(0.5, 1.5, n)
    if case == "per_system_final_times":
        r = _gpu_case(st, n, lambda ta: ta.propagate_until(tf))
        assert np.array_equal(r["time_hi"], tf) and np.unique(r["n_steps"]).size > 1
    elif case in ("max_delta_t_below", "max_delta_t_straddles"):
        h0 = _gpu_natural_step(st)
        mdt = (0.5 if case == "max_delta_t_below" else 2.0) * h0
        tf = 12.0 * h0 * np.random.RandomState(1).uniform(0.5, 1.5, n)
        r = _gpu_case(st, n, lambda ta: ta.propagate_until(tf, max_delta_t=mdt))
        assert np.array_equal(r["time_hi"], tf) and np.all(r["max_h"] <= mdt)
    elif case == "backward":
        r = _gpu_case(st, n, lambda ta: ta.propagate_until(-tf))
        assert np.array_equal(r["time_hi"], -tf) and np.all(r["last_h"] < 0)
    else:
        # (A non-finite VALUE is ordinary data. What the other systems of the batch do once one of them reports it is the
        # integrator's batch semantics, the same for both kernels: compared like everything else.)
        st2 = st.copy()
        st2[0, 2049] = np.inf
        r = _gpu_case(st2, n, lambda ta: ta.propagate_until(tf))
        assert r["outcome"][2049] == int(hy.taylor_outcome.err_nf_state)
        assert np.count_nonzero(r["outcome"] == int(hy.taylor_outcome.err_nf_state)) == 1


@pytest.mark.gpu
def test_gpu_refill_meets_the_plain_path():
    """40 003 systems with 1e-2 perturbations: the queue outlasts the resident slots, so systems are retired and replaced
    while their neighbours take plain steps."""
    n = 40003
    st = configs.outer_ss_state(n, perturb=1e-2, seed=91)
    tf = np.random.RandomState(5).uniform(2.0, 45.0, n)
    r = _gpu_case(st, n, lambda ta: ta.propagate_until(tf))
    assert np.array_equal(r["time_hi"], tf) and r["n_steps"].max() >= 4 * max(1, int(np.median(r["n_steps"]))) // 3
