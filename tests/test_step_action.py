"""step_action: expression-defined step callbacks applied on the device. Host half: the object, the
checks against the system, the generated module (hiprtc cross-compiles without a GPU) and the C++ program written
against <heyoka/callback/step_action.hpp>; the device half of that program is marked gpu. The numbers are checked in
tests/test_step_action_gpu.py."""
import copy
import ctypes
import os
import subprocess

import pytest

import heyoka_amd as hy
from heyoka_amd import _lib, codegen_check, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_step_action")


def osc():
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -x)], x, v


def test_constructor_and_repr():
    _, x, v = osc()
    a = hy.step_action({v: 0.5 * v, x: v}, stop_when=hy.gt(x, 2.0))
    assert repr(a).startswith("step_action({v: ") and ", x: v}" in repr(a) and "stop_when=" in repr(a)
    # A list of pairs keeps its order; the condition alone is an action too.
    b = hy.step_action([(x, v), (v, x)])
    assert repr(b) == "step_action({x: v, v: x})"
    c = hy.step_action(stop_when=hy.gt(x, 2.0))
    assert repr(c).startswith("step_action({}, stop_when=")
    # Copies are independent objects with the same text.
    for d in (copy.copy(a), copy.deepcopy(a)):
        assert d is not a and d._h != a._h and repr(d) == repr(a)
    with pytest.raises(ValueError, match="neither assignments nor a stop condition"):
        hy.step_action()
    with pytest.raises(ValueError, match="neither assignments nor a stop condition"):
        hy.step_action({})
    with pytest.raises(ValueError, match="of an assignment of a step action is not a variable"):
        hy.step_action({x + v: v})
    with pytest.raises(ValueError, match="takes a dict or a list"):
        hy.step_action([(x, v, v)])


def test_checks_against_the_system():
    """Made when the action first meets an integrator - the propagate call or a direct call - before anything runs."""
    sys_, x, v = osc()
    w = hy.make_vars("w")
    ta = hy.taylor_adaptive_batch(sys_, None, 4)
    bad = [
        (hy.step_action({w: v}), "The left-hand side 'w' of an assignment of a step action is not a state variable"),
        (hy.step_action([(v, x), (v, v)]), "The state variable 'v' is assigned more than once by a step action"),
        (hy.step_action({v: w * v}), "uses the variable 'w', which is not a state variable of the system"),
        (hy.step_action({v: v}, stop_when=hy.gt(w, 1.0)), "The stop condition of a step action uses the variable 'w'"),
        (hy.step_action({v: hy.par[0] * v}), r"A step action uses par\[0\], but the integrator has 0 parameter"),
    ]
    for act, msg in bad:
        with pytest.raises(ValueError, match=msg):
            act(ta)
        with pytest.raises(ValueError, match=msg):
            ta.propagate_until(1.0, callback=act)
        with pytest.raises(ValueError, match=msg):
            ta.propagate_for(1.0, callback=[lambda t: True, act])
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid([0.0, 1.0], callback=act)
        with pytest.raises(ValueError, match=msg):
            ta.step_action_module(act)
    # One parameter is enough for par[0], not for par[1].
    tp = hy.taylor_adaptive_batch([(x, v), (v, -hy.par[0] * x)], None, 4)
    tp.step_action_module(hy.step_action({v: hy.par[0] * v}))
    with pytest.raises(ValueError, match=r"uses par\[1\], but the integrator has 1 parameter"):
        tp.step_action_module(hy.step_action({v: hy.par[1] * v}))


def test_c_abi_round_trip():
    lib = _lib.lib
    _, x, v = osc()
    half_v = 0.5 * v  # (kept alive across the C calls)
    larr = (ctypes.c_void_p * 1)(v._h)
    rarr = (ctypes.c_void_p * 1)(half_v._h)
    cond = hy.gt(x, 2.0)
    h = lib.hy_step_action_new(larr, rarr, 1, cond._h)
    assert h
    txt = _lib.take_str(lib.hy_step_action_str(h))
    assert txt == repr(hy.step_action({v: 0.5 * v}, stop_when=hy.gt(x, 2.0)))
    h2 = lib.hy_step_action_clone(h)
    assert h2 and h2 != h and _lib.take_str(lib.hy_step_action_str(h2)) == txt
    lib.hy_step_action_free(h)
    assert _lib.take_str(lib.hy_step_action_str(h2)) == txt
    lib.hy_step_action_free(h2)
    # The condition alone (n == 0), and the two failures of the constructor.
    h3 = lib.hy_step_action_new(None, None, 0, cond._h)
    assert h3
    lib.hy_step_action_free(h3)
    assert not lib.hy_step_action_new(None, None, 0, None)
    assert "neither assignments nor a stop condition" in lib.hy_last_error().decode()
    x_plus_v = x + v
    bad = (ctypes.c_void_p * 1)(x_plus_v._h)
    assert not lib.hy_step_action_new(bad, rarr, 1, None)
    assert "is not a variable" in lib.hy_last_error().decode()
    # The ready-made member: -1 and the message on an error.
    ta = hy.taylor_adaptive_batch(osc()[0], None, 4)
    w = hy.make_vars("w")
    act = hy.step_action({w: v})
    assert lib.hy_step_action_call(ta._h, act._h) == -1
    assert "is not a state variable" in lib.hy_last_error().decode()
    assert lib.hy_step_action_call(ta._h, None) == -1


def pendulum_case():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.par[1] * hy.sin(x))]
    return sys_, hy.step_action({v: v + hy.par[0] * hy.cos(hy.time)}, stop_when=hy.gt(v * v, 100.0))


def outer_ss_case():
    sys_ = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
    vs = {repr(e): e for e in hy._to_sys(sys_).vars}
    scale = 1.0 + 1e-12
    return sys_, hy.step_action({vs[n]: scale * vs[n] for n in ("vx_1", "vy_1", "vz_1")})


def osc_case():
    sys_, x, v = osc()
    return sys_, hy.step_action({x: v, v: x}, stop_when=hy.gt(x * x + v * v, 4.0))


@pytest.mark.parametrize("case", [osc_case, pendulum_case, outer_ss_case])
def test_source_compiles_without_scratch(case):
    sys_, act = case()
    src = hy.step_action_source(sys_, act)
    assert 'extern "C" __global__ void __launch_bounds__(256) hy_step_action(' in src
    # Plain HIP C++: no LDS, no inline assembly; last_h is the first load of the kernel.
    assert "__shared__" not in src and "asm" not in src.split("hy_step_action(const hy_sa_args a)")[1]
    body = src.split("hy_step_action(const hy_sa_args a)")[1]
    assert body.index("a.last_h[s] == 0.0") < body.index("a.state[")
    co = hy.hiprtc_compile(src)
    assert co[:4] == b"\x7fELF"
    res = codegen_check.kernel_resources(co, kernel="hy_step_action")
    assert res is not None
    assert res["scratch_bytes_per_lane"] == 0 and res["vgpr_spill"] == 0 and res["sgpr_spill"] == 0, res
    assert res["lds_bytes"] == 0, res


def test_module_in_an_integrator_and_sources_untouched():
    """The module of an action is kept in the integrator (and its copies recompile lazily), and the stepper's source is
    byte-identical before and after the action met the integrator (without a GPU the meeting is step_action_module(), what
    a propagate call does first). The event-detection source is a function of (order, number of events) alone - no action
    can reach it; that it is the pinned text is tested in tests/test_event_recorder.py."""
    sys_, x, v = osc()
    act = hy.step_action({v: 0.5 * v}, stop_when=hy.gt(x, 2.0))
    ta = hy.taylor_adaptive_batch(sys_, None, 8, nt_events=[hy.nt_event(v, hy.native_event_counter())])
    stepper = ta.hip_source
    src, co = ta.step_action_module(act)
    assert src == hy.step_action_source(sys_, act) and co[:4] == b"\x7fELF"
    assert ta.step_action_module(copy.copy(act))[0] == src
    assert ta.hip_source == stepper
    tb = copy.deepcopy(ta)
    assert tb.step_action_module(act)[0] == src
    assert tb.hip_source == stepper
    assert ta.n_stopped_by_action == 0 and ta.last_callback_path == 0


def _build_cpp():
    """tests/cpp/test_step_action.cpp, compiled the way tests/test_variational.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_step_action.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_step_action_host_half():
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_cpp_step_action_on_gpu():
    out = subprocess.run([_build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
