"""callback::angle_reducer without a GPU: the C++ class (construction, copy / move, stream text, error messages), the
arithmetic of the reduction - the host function and the text of the DEVICE helper compiled for the host - against numpy's
unfused x - twopi * floor(x / twopi) bit for bit, the generated sources of the stepper variants with the reduction fused
in, and one fused propagation of the multi-class wave-cluster kernel under the wavefront emulator of tests/emu."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import emu  # noqa: E402
import heyoka_oracle as ho  # noqa: E402

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import _lib  # noqa: E402
from heyoka_amd import mixed_models as mm  # noqa: E402

EPS = 2.220446049250313e-16
TWOPI = float.fromhex("0x1.921fb54442d18p+2")
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_angle_reducer")


def build_cpp():
    src = os.path.join(ROOT, "tests", "cpp", "test_angle_reducer.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def np_reduce(x):
    x = np.asarray(x, dtype=np.float64)
    return x - TWOPI * np.floor(x / TWOPI)


def pendula():
    x0, x1, v0, v1 = hy.make_vars("x0", "x1", "v0", "v1")
    return [(x0, v0), (x1, v1), (v0, -hy.sin(x0)), (v1, -hy.sin(x1))], (x0, x1, v0, v1)


def test_cpp_class_construction_copy_move_stream_and_error_messages():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "angle_reducer host checks OK" in out.stdout


def test_python_class_repr_and_errors():
    (x0, x1, v0, _v1) = pendula()[1]
    assert repr(hy.callback.angle_reducer([x1, x0])) == "Angle reducer: {x0, x1}"
    assert repr(hy.callback.angle_reducer()) == "Angle reducer (default constructed)"
    with pytest.raises(ValueError) as e:
        hy.callback.angle_reducer([])
    assert str(e.value) == "The list of expressions passed to the constructor of angle_reducer cannot be empty"
    with pytest.raises(ValueError) as e:
        hy.callback.angle_reducer([x0, v0 + 1.0])
    assert str(e.value) == "The list of expressions passed to the constructor of angle_reducer can contain only variables"
    import copy

    assert repr(copy.deepcopy(hy.callback.angle_reducer([v0]))) == "Angle reducer: {v0}"


VALUES = np.array([0.0, 1e-300, -1e-300, 1e-20, -1e-20, np.nextafter(2 * np.pi, np.inf), np.nextafter(2 * np.pi, -np.inf),
                   100.5, -100.5, 1e15, -1e15])


def _device_helper_on_the_host(contract):
    """The text of the __device__ helper the kernels call, compiled for the host like the emulated kernels - with
    contraction allowed and FMA instructions available when `contract`: the helper must keep the product and the difference
    apart by itself."""
    src = _lib.take_str(_lib.lib.hy_angle_reduce_source())
    helper = src[: src.index("struct hy_ar_kargs")]
    assert "hy_angle_red(double x)" in helper
    text = ('#define HY_NO_NMAX 1\n#define HY_HOST_EMU 1\n#include "wave_emu.hpp"\n' + helper.replace('"+v"(', '"+x"(')
            + '\nextern "C" double red(double x) { return hy_angle_red(x); }\n')
    os.makedirs(emu.BUILD, exist_ok=True)
    cpp = os.path.join(emu.BUILD, "angle_red_%d.cpp" % int(contract))
    so = cpp[:-4] + ".so"
    with open(cpp, "w") as f:
        f.write(text)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-w", "-mfma", "-I", emu.HERE,
                           "-ffp-contract=" + ("fast" if contract else "off"), "-o", so, cpp])
    lib = ctypes.CDLL(so)
    lib.red.restype = ctypes.c_double
    lib.red.argtypes = [ctypes.c_double]
    return lib.red


def test_reduction_arithmetic_matches_numpy_bit_for_bit():
    ref = np_reduce(VALUES)
    # (The tiny negative arguments give exactly twopi - the one point where the map is not idempotent.)
    assert ref[2] == TWOPI and ref[4] == TWOPI and np_reduce(ref[2]) == 0.0
    fns = {"host": _lib.lib.hy_angle_reduce_host, "device helper": _device_helper_on_the_host(False),
           "device helper, contraction on": _device_helper_on_the_host(True)}
    for name, fn in fns.items():
        got = np.array([fn(float(v)) for v in VALUES])
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (name, got, ref)
        assert fn(float("inf")) == float("inf") and fn(float("-inf")) == float("-inf") and np.isnan(fn(float("nan"))), name
        rng = np.random.RandomState(3)
        xs = np.concatenate([rng.uniform(-50.0, 50.0, 2000), rng.uniform(-1e6, 1e6, 2000)])
        got = np.array([fn(float(v)) for v in xs])
        assert np.array_equal(got.view(np.uint64), np_reduce(xs).view(np.uint64)), name


CALL = re.compile(r"(?<!double )hy_angle_red\(")


def _stepper(src):
    """The text of the kernel hy_taylor alone (the straight-line generator emits a second kernel which streams the Taylor
    coefficients out)."""
    a = src.index("hy_taylor(const hy_kargs a)")
    b = src.find("hy_taylor_tc(const hy_kargs a)")
    return src[a: b if b > a else len(src)]


def _strip(src):
    """A fused variant with everything the reduction added taken out again."""
    helper = _lib.take_str(_lib.lib.hy_angle_reduce_source())
    helper = helper[: helper.index("struct hy_ar_kargs")].rstrip("\n") + "\n"
    assert helper in src
    src = src.replace(helper, "")
    src = re.sub(r"^ *if \(i == \d+u\) res = hy_angle_red\(res\);\n", "", src, flags=re.M)
    src = re.sub(r"^const bool sred\d+ = .*\n", "", src, flags=re.M)
    src = re.sub(r"sred\d+ \? hy_angle_red\(res\) : res", "res", src)
    return re.sub(r"hy_angle_red\((\w+)\)", r"\1", src)


@pytest.mark.parametrize("family", ["unrolled", "staged", "hbm_tape", "multi_class"])
def test_generated_sources_of_the_fused_variants(family, monkeypatch):
    """Without a list the source is the one without the feature (no trace of the helper; and a variant with the added text
    taken out again IS that source); with a list the helper is called once per flagged variable and never for another."""
    if family in ("staged", "hbm_tape"):
        monkeypatch.setenv("HEYOKA_AMD_EMIT_MODE", "table")
        monkeypatch.setenv("HEYOKA_AMD_TABLE_LDS", "1" if family == "staged" else "0")
    if family == "multi_class":
        ta = hy.taylor_adaptive_batch(mm.sine_lattice(hy, 16), None, 64)
        want, flagged = "classes of clusters", [1, 5, 17]
    else:
        ta = hy.taylor_adaptive_batch(pendula()[0], None, 64, **({"emitter": "unrolled"} if family == "unrolled" else {}))
        want, flagged = {"unrolled": "unrolled", "staged": "table mode (staged)", "hbm_tape": "tape in HBM"}[family], [0, 1]
    assert want in ta.hip_source_mode, ta.hip_source_mode
    base = ta.hip_source
    assert "hy_angle_red" not in base
    for idx in (flagged, flagged[:1], [3]):
        src, why = ta.angle_reduce_variant_source(idx)
        assert src and why == ""
        assert _strip(src) == base
        k = _stepper(src)
        if family == "multi_class":
            # (One guarded call per round of state variables with a flagged member: lane l holds variable r * 16 + l.)
            assert len(CALL.findall(k)) == len({i // 16 for i in idx})
            for i in idx:
                assert re.search(r"const bool sred%d = svalid%d && \(.*svi%d == %du" % (i // 16, i // 16, i // 16, i), k)
            assert len(re.findall(r"svi\d+ == \d+u", k)) == len(idx)
        else:
            assert len(CALL.findall(k)) == len(idx)
            if family == "unrolled":
                for i in range(4):
                    assert (("x%d = hy_angle_red(x%dn);" % (i, i)) in k) == (i in idx)
            else:
                for i in range(4):
                    assert (("if (i == %du) res = hy_angle_red(res);" % i) in k) == (i in idx)
    with pytest.raises(ValueError):
        ta.angle_reduce_variant_source([ta.dim])


def test_generators_without_a_fused_variant_decline_with_a_reason():
    from heyoka_amd import configs

    oss = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
    ta = hy.taylor_adaptive_batch(oss, None, 8, high_accuracy=True)
    assert "cluster mode v5" in ta.hip_source_mode
    src, why = ta.angle_reduce_variant_source([0])
    assert src == "" and "no fused angle reduction" in why and "v5" in why


def test_emulated_fused_step_of_the_multi_class_cluster_kernel():
    """The 16-site sine lattice (the smallest chain the planner gives to the multi-class wave-cluster generator: shorter
    ones run as straight-line code), angles offset by +40, 5 systems (one full group of 4 per wavefront and a partial one).
    The emulator runs this kernel one step per launch (in a propagate-mode launch the systems of a wavefront leave the step
    loop at different iterations, which its rendezvous points do not model), so the fused variant is stepped in lock-step:
    every sweep must give, bit for bit, what the unfused kernel gives with numpy reducing the flagged angles afterwards -
    and the oracle stepped the same way agrees to 1e3 eps per step, the bound of the single-step comparison of the emulated
    kernels (the step size goes through exp(log()) in the kernel and pow() in the oracle)."""
    ns, n, n_sweeps = 16, 5, 4
    flagged = list(range(0, ns, 2)) + [ns - 1]
    st = mm.sine_lattice_state(ns, n, seed=3)
    st[:ns] += 40.0
    ta = hy.taylor_adaptive_batch(mm.sine_lattice(hy, ns), None, 64)
    assert "2 classes of clusters" in ta.hip_source_mode
    spw = (ta.order + 1) * 4 * 64
    src, why = ta.angle_reduce_variant_source(flagged)
    assert src, why
    fused, base = emu.EmulatedKernel(src), emu.EmulatedKernel(ta.hip_source)
    ora = ho.OracleIntegrator(mm.sine_lattice(ho, ns), st, n)
    cur_f, cur_b, t = st.copy(), st.copy(), np.zeros(n)
    lim = np.array([np.inf, 0.01, 0.0, np.inf, np.inf])  # (system 2 takes zero-length steps: reduced all the same)
    for sweep in range(n_sweeps):
        rf = fused.run(cur_f, t, np.zeros(n), mode=0, lim=lim, scratch_per_wave=spw)
        rb = base.run(cur_b, t, np.zeros(n), mode=0, lim=lim, scratch_per_wave=spw)
        cur_b = rb["state"]
        cur_b[flagged] = np_reduce(cur_b[flagged])
        cur_f = rf["state"]
        assert np.array_equal(cur_f.view(np.uint64), cur_b.view(np.uint64)), sweep
        assert np.array_equal(rf["last_h"], rb["last_h"]) and np.array_equal(rf["time_hi"], rb["time_hi"])
        assert np.all(cur_f[flagged] >= 0.0) and np.all(cur_f[flagged] <= TWOPI)
        t = rf["time_hi"]
        ora.step(max_delta_ts=lim)
        os_ = ora.state.reshape(2 * ns, n)
        os_[flagged] = np_reduce(os_[flagged])
        d = np.abs(cur_f - os_)
        d[flagged] = np.minimum(d[flagged], TWOPI - d[flagged])  # (on the circle)
        assert np.max(d / np.maximum(1.0, np.abs(os_))) <= 1e3 * EPS * (sweep + 1), sweep
    assert t[2] == 0.0 and np.all(t[[0, 3, 4]] > 0.0)
    unflagged = [i for i in range(ns) if i not in flagged]
    assert np.all(cur_f[unflagged] > 30.0)
