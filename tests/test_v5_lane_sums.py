"""The lane-reduced sums of the one-lane-per-pair stepper ("v5"): with the reactions fused into the acceleration sums, the
terms of the plain sums of the later rounds (the first body of every pair) sit in a register of the first-round lanes, and
three row_shr steps add them there instead of five LDS reads per order. The arithmetic and its order are those of the
pairwise sum rule, so the kernel must give bit for bit the results of the kernel with the item switched off
(HEYOKA_AMD_V5_OPTS=nolanesum, which restores the text of before). CPU: the generated source under the wavefront emulator
of tests/emu (which implements row_shr) and static counts of the step loop; -m gpu: the same comparisons on 4 096 systems."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import codegen_check, configs  # noqa: E402
from test_v5_lds_diet import VARIANTS, _build, _gpu_outputs, _state  # noqa: E402

OFF = "nolanesum"
PHRASE = "later sums reduced across the lanes of the first round"
STEP_KEYS = ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "tc")
PROP_KEYS = ("state", "time_hi", "time_lo", "last_h", "outcome", "n_steps", "min_h", "max_h")


def _build_default_masses(opts):
    old = os.environ.get("HEYOKA_AMD_V5_OPTS")
    os.environ["HEYOKA_AMD_V5_OPTS"] = opts
    try:
        return hy.taylor_adaptive_batch(hy.model.nbody(6), None, 64, high_accuracy=True)
    finally:
        if old is None:
            os.environ.pop("HEYOKA_AMD_V5_OPTS", None)
        else:
            os.environ["HEYOKA_AMD_V5_OPTS"] = old


def _emulated_bit_comparison(new, off, st_of, horizon, name):
    """One step with all Taylor coefficients of 11 systems, and propagate_until() with per-system final times on 5 systems
    more than one workgroup keeps in flight (the retire / refill path)."""
    import emu

    kn, ko = emu.EmulatedKernel(new.hip_source), emu.EmulatedKernel(off.hip_source)
    n = 11
    st = st_of(n)
    rows = st.shape[0] * (new.order + 1)
    rn, ro = [k.run(st, np.zeros(n), np.zeros(n), mode=0, lim=np.full(n, np.inf), want_tc_rows=rows) for k in (kn, ko)]
    assert np.all(rn["last_h"] > 0) and np.isfinite(rn["tc"]).all() and np.any(rn["tc"][-1] != 0.0)
    for key in STEP_KEYS:
        assert np.array_equal(rn[key], ro[key]), (name, "step", key)
    n = kn.block // kn.lanes_per_system + 5
    st = st_of(n)
    tf = horizon * np.random.RandomState(1).uniform(0.5, 1.5, n)
    pn, po = [k.run(st, np.zeros(n), np.zeros(n), mode=1, tfin=tf, max_grid=1) for k in (kn, ko)]
    assert np.array_equal(pn["time_hi"], tf) and np.unique(pn["n_steps"]).size > 1
    for key in PROP_KEYS:
        assert np.array_equal(pn[key], po[key]), (name, "propagation", key)


def _check_takes_the_path(new, off):
    assert PHRASE in new.hip_source_mode and PHRASE not in off.hip_source_mode, (new.hip_source_mode, off.hip_source_mode)
    assert new.hip_source != off.hip_source
    # (Three row_shr steps per order on the existing helper; no hand-written EXEC manipulation, no assembly for them.)
    assert new.hip_source.count("hy_dpp<0x111>(") == 2 * new.order and new.hip_source.count("hy_dpp<0x112>(") == new.order
    assert "hy_dpp<0x11" not in off.hip_source
    assert "s_mov_b64 exec" not in new.hip_source and "saveexec" not in new.hip_source
    assert new.hip_source.count("asm") == off.hip_source.count("asm")


def test_emulated_lane_sums_are_bit_identical_to_the_kernel_without_them():
    """The headline (outer Solar System, 16 lanes per system) takes the path, and every output of a step and of a
    propagation with retire / refill equals the flag-off kernel's."""
    new, off = _build(6, ""), _build(6, OFF)
    assert "lanes per system: 16," in new.hip_source_mode
    _check_takes_the_path(new, off)
    # (The model of the slab's bank conflicts was run again under the new reader lanes.)
    assert "slab layout: 0 conflict cycles per step in the model" in new.hip_source_mode, new.hip_source_mode
    assert "snew < N" in new.hip_source
    _emulated_bit_comparison(new, off, lambda n: _state(6, n), VARIANTS["outer_ss_16_lanes"][2], "outer_ss_16_lanes")


@pytest.mark.parametrize("name", sorted(VARIANTS) + ["nbody6_default_masses"])
def test_every_variant_takes_the_path_bit_for_bit_or_keeps_its_text(name):
    """Which variants take the path is reported, not asserted (several have a single round or sums of another length): one
    which does is compared bit for bit, one which does not has the same source with and without the flag."""
    if name == "nbody6_default_masses":
        new, off = _build_default_masses(""), _build_default_masses(OFF)
        st_of, horizon = (lambda n: _state(6, n)), 2.0
    else:
        nb, _, horizon = VARIANTS[name]
        new, off = _build(nb, ""), _build(nb, OFF)
        st_of = lambda n: _state(nb, n)  # noqa: E731
    takes = PHRASE in new.hip_source_mode
    print("%s: %s" % (name, "lane-reduced sums" if takes else "declined, text unchanged"))
    if not takes:
        assert new.hip_source == off.hip_source
        return
    _check_takes_the_path(new, off)
    _emulated_bit_comparison(new, off, st_of, horizon, name)


def test_the_stepper_with_events_keeps_its_text():
    x1, x2 = hy.make_vars("x_1", "x_2")
    src = []
    for opts in ("", OFF):
        ta = _build(6, opts, nt_events=[hy.nt_event((x1 - x2) * (x1 - x2) - 4.0, lambda *a: None)])
        assert "events:" in ta.hip_source_mode and PHRASE not in ta.hip_source_mode, ta.hip_source_mode
        src.append(ta.hip_source)
    assert src[0] == src[1]


_STATIC_CHILD = r"""
import json, os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "profiles", "experiments")]
import isa_count
from heyoka_amd import codegen_check
from test_v5_lds_diet import _build
isa_count.OBJDUMP = codegen_check.find_objdump() or isa_count.OBJDUMP
new, off = _build(6, ""), _build(6, sys.argv[2])
print(json.dumps({"new": isa_count.step_loop_counts(new.code_object), "off": isa_count.step_loop_counts(off.code_object),
                  "res": codegen_check.kernel_resources(new.code_object)}))
"""


def test_static_counts_of_the_step_loop():
    """Both kernels compiled for gfx950, the step loop counted as profiles/experiments/isa_count.py does. Relative to the
    flag-off kernel built next to it (the compiler differs between machines): at least 100 LDS reads less per step (5 reads
    at 20 orders), no more FP64 instructions and no more LDS writes; and the resources of the headline. The two compilations
    run in a process of their own, so that both counts come from one compiler whatever ran before: a process which has
    imported torch compiles with the hiprtc inside PyTorch, not ROCm's, and the two allocate registers differently
    (profiles/HISTORY.md, "Two compilers")."""
    import json
    import subprocess

    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k != "HEYOKA_AMD_V5_OPTS"}
    out = subprocess.run([sys.executable, "-c", _STATIC_CHILD, root, OFF], env=env, capture_output=True, text=True, check=True).stdout
    d = json.loads(out.strip().split("\n")[-1])
    cn, co, res = d["new"], d["off"], d["res"]
    print("step loop, new:", cn, "\nstep loop, off:", co, "\nresources:", res)
    assert cn["lds_read"] <= co["lds_read"] - 100, (cn, co)
    assert cn["valu_fp64"] <= co["valu_fp64"], (cn, co)
    assert cn["lds_write"] <= co["lds_write"], (cn, co)
    assert res["vgpr_total"] == 256 and res["waves_per_simd_by_registers"] == 2, res
    assert res["vgpr_spill"] <= 18 and res["lds_bytes"] <= 160 * 1024, res


@pytest.mark.gpu
def test_gpu_lane_sums_are_bit_identical_and_deterministic():
    """4 096 systems on the GPU: one step with all Taylor coefficients and a propagate_until() with per-system final times,
    default kernel, flag-off kernel and the default kernel again on a fresh integrator: every output array_equal."""
    n = 4096
    st = configs.outer_ss_state(n, perturb=1e-3, seed=42)
    tf = 30.0 * np.random.RandomState(1).uniform(0.5, 1.5, n)
    new, off, again = _build(6, "", st, n), _build(6, OFF, st, n), _build(6, "", st, n)
    _check_takes_the_path(new, off)
    assert again.hip_source == new.hip_source
    steps, props = [], []
    for ta in (new, off, again):
        ta.step(write_tc=True)
        steps.append(_gpu_outputs(ta, False))
    assert np.all(steps[0]["last_h"] > 0) and np.isfinite(steps[0]["tc"]).all() and np.any(steps[0]["tc"][-1] != 0.0)
    for ta in (new, off, again):
        ta.propagate_until(tf)
        props.append(_gpu_outputs(ta, True))
    assert np.array_equal(props[0]["time_hi"], tf) and np.unique(props[0]["n_steps"]).size > 1
    for outs, what in ((steps, "step"), (props, "propagation")):
        for key in outs[0]:
            assert np.array_equal(outs[0][key], outs[1][key]), (what, "flag off", key)
            assert np.array_equal(outs[0][key], outs[2][key]), (what, "second run", key)
