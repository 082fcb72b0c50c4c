"""Terminal-event actions (hy.event_action): a terminal callback defined by assignments
``state variable <- expression``, applied by the generated kernel hy_ev_action - behind the device-side event handling when
every event of the integrator is library-side, at its place in the host loop otherwise.

CPU: construction and validation, where the events are applied, the action module (compiles for gfx950, reads before it
writes), the sources which must not change. GPU: the action against the same integrator with a Python callback doing the
same operation (bit for bit: one rounding on either side), against the CPU oracle (tolerance of the event parity tests of
tests/test_gpu_parity.py: rel_err() <= 1e5 eps for the small systems), against hy.cfunc of the same expressions (bit for
bit: the yardstick), and the invariances - first terminal event only, the host-loop path, independent semantics, batch
size, copies."""
import copy
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
import heyoka_oracle as ho
from heyoka_amd import _lib, configs
from conftest import EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OC = hy.taylor_outcome
NEG_HY, NEG_HO = hy.event_direction.negative, ho.DIR_NEGATIVE
POS_HY = hy.event_direction.positive
BOUNCE = -0.8
# The tolerance of test_events_batch_vs_oracle (tests/test_gpu_parity.py) on the states of the small systems.
STATE_TOL = 1e5 * EPS


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def _osc(m):
    if m is ho:
        x, v = ho.var("x"), ho.var("v")
        return [(x, v), (v, -1.0 * x)], x, v
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -x)], x, v


def _bouncer(n=3, cb="action", extra_t=(), nt=(), state=None, **kw):
    """x' = v, v' = -x with the terminal event x = 0 (downwards) whose callback is the action {v: -0.8 v} ("action"), a
    Python function doing the same through the public interface ("python") or a counter ("counter")."""
    sys_, x, v = _osc(hy)
    if cb == "action":
        cb = hy.event_action({v: BOUNCE * v})
    elif cb == "python":
        def cb(ta, d_sgn, i):
            ta.state_data()[1, i] *= BOUNCE
            return True
    elif cb == "counter":
        cb = hy.native_event_counter()
    return hy.taylor_adaptive_batch(sys_, state, n, t_events=[hy.t_event(x, callback=cb, direction=NEG_HY)] + list(extra_t),
                                    nt_events=list(nt), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_construction_repr_and_copies():
    x, v = hy.make_vars("x", "v")
    a = hy.event_action({v: BOUNCE * v})
    assert repr(a).startswith("event_action({v: ") and "0.8" in repr(a)
    # A list of pairs keeps its order.
    b = hy.event_action([(v, x), (x, v)])
    assert re.match(r"event_action\(\{v: x, x: v\}\)", repr(b)), repr(b)
    for c in (copy.copy(a), copy.deepcopy(a)):
        assert isinstance(c, hy.event_action) and repr(c) == repr(a) and c._h != a._h
    with pytest.raises(ValueError, match="empty list of assignments"):
        hy.event_action({})
    with pytest.raises(ValueError, match="empty list of assignments"):
        hy.event_action([])
    with pytest.raises(ValueError, match="is not a variable"):
        hy.event_action([(x + v, x)])
    with pytest.raises(ValueError, match="pairs"):
        hy.event_action([(x, v, x)])


def test_validation_against_the_system():
    sys_, x, v = _osc(hy)
    q = hy.make_vars("q")

    def build(assignments):
        return hy.taylor_adaptive_batch(sys_, None, 3, t_events=[hy.t_event(x, callback=hy.event_action(assignments))])

    with pytest.raises(ValueError, match=r"'v' is assigned more than once by an event action \(terminal event 0\)"):
        build([(v, 1.0 * x), (v, 2.0 * x)])
    with pytest.raises(ValueError, match="left-hand side 'q' .* is not a state variable of the system"):
        build({q: 1.0 * x})
    with pytest.raises(ValueError, match="uses the variable 'q', which is not a state variable of the system"):
        build({v: q * x})
    with pytest.raises(ValueError, match=r"uses par\[0\], but the system and its event equations have 0 parameter"):
        build({v: hy.par[0] * x})
    # Numbers, parameters the system has, the time and plain copies are fine.
    ta = hy.taylor_adaptive_batch([(x, v), (v, -hy.par[0] * x)], None, 3,
                                  t_events=[hy.t_event(x, callback=hy.event_action({x: 1.5, v: x + hy.par[0] * hy.time}))])
    assert ta.n_event_actions == 1


def test_the_c_abi_handle_and_marker():
    lib = _lib.lib
    x, v = hy.make_vars("x", "v")
    rhs = BOUNCE * v
    larr, rarr = (ctypes.c_void_p * 1)(v._h), (ctypes.c_void_p * 1)(rhs._h)
    h = lib.hy_event_action_new(larr, rarr, 1)
    assert h
    h2 = lib.hy_event_action_clone(h)
    assert h2 and h2 != h
    assert _lib.take_str(lib.hy_event_action_str(h)) == _lib.take_str(lib.hy_event_action_str(h2)) == repr(hy.event_action({v: rhs}))
    assert not lib.hy_event_action_new(larr, rarr, 0) and "empty list" in _lib.last_error()
    # The integrator owns a copy: the handle may go right after the construction.
    sys_ = hy.model.pendulum()
    te = (_lib.TEvent * 1)(_lib.TEvent(x._h, ctypes.cast(lib.hy_event_action_t, _lib.T_EVENT_CB), ctypes.c_void_p(h), 0, -1.0))
    t = lib.hy_tab_create_with_events(sys_._h, None, 0, 4, None, te, 1, None, 0)
    assert t, _lib.last_error()
    lib.hy_event_action_free(h)
    assert lib.hy_tab_events_on_device(t) == 1 and lib.hy_tab_n_event_actions(t) == 1
    t2 = lib.hy_tab_copy(t)
    lib.hy_tab_free(t)
    assert t2 and lib.hy_tab_events_on_device(t2) == 1 and lib.hy_tab_n_event_actions(t2) == 1
    src = ctypes.c_void_p()
    assert lib.hy_tab_event_action_module(t2, ctypes.byref(src), None, None) == 0
    assert "hy_ev_action" in _lib.take_str(src.value)
    # The marker without a handle, and on an integrator the action does not belong to, reports an error.
    assert lib.hy_event_action_t(t2, 0, 0, None) == 0 and "hy_event_action handle" in _lib.last_error()
    lib.hy_tab_free(t2)
    lib.hy_event_action_free(h2)
    plain = hy.taylor_adaptive_batch(hy.model.pendulum(), None, 4)
    with pytest.raises(ValueError, match="does not belong to a terminal event of this integrator"):
        hy.event_action({v: rhs})(plain, 0, 0)
    # An integrator without actions has no action module.
    with pytest.raises(ValueError, match="no event actions"):
        plain.event_action_module()


@pytest.mark.parametrize("semantics", [None, "independent"])
def test_nativeness(semantics):
    """Actions, counters and recorders: every event library-side, under either semantics; one Python callback and the
    integrator keeps the host loop; a copy keeps the actions."""
    sys_, x, v = _osc(hy)
    lib_side = dict(extra_t=[hy.t_event(x - 2.0, callback=hy.native_event_counter()), hy.t_event(v - 2.0, callback=hy.native_event_recorder())],
                    nt=[hy.nt_event(v, hy.native_event_recorder()), hy.nt_event(x - 0.5, hy.native_event_counter())])
    ta = _bouncer(batch_semantics=semantics, **lib_side)
    assert ta.event_stats["events_on_device"] is True and ta.n_event_actions == 1
    for c in (copy.copy(ta), copy.deepcopy(ta)):
        assert c.event_stats["events_on_device"] is True and c.n_event_actions == 1
        assert c.event_action_module()[0] == ta.event_action_module()[0]
    lib_side["nt"] = lib_side["nt"] + [hy.nt_event(x - 0.25, lambda *a: None)]
    tb = _bouncer(batch_semantics=semantics, **lib_side)
    assert tb.event_stats["events_on_device"] is False and tb.n_event_actions == 1
    # A plain stop next to an action: library-side under the independent semantics only.
    tc = _bouncer(batch_semantics=semantics, extra_t=[hy.t_event(x - 1.0)])
    assert tc.event_stats["events_on_device"] is (semantics == "independent")


def test_the_action_module_compiles_and_no_other_text_changes():
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    x, v = hy.make_vars("x", "v")
    for emitter in (None, "table"):
        a, c = _bouncer(emitter=emitter), _bouncer(cb="counter", emitter=emitter)
        assert a.hip_source == c.hip_source and a.hip_source_mode == c.hip_source_mode
        assert "hy_ev_action" not in a.hip_source
    src, code = a.event_action_module()
    assert "hy_ev_action" in src and code[:4] == b"\x7fELF"
    assert hy.hiprtc_compile(src)[:4] == b"\x7fELF"
    # The event-detection module is a function of (order, number of events) alone.
    det = _lib.take_str(_lib.lib.hy_event_detection_source(a.order, 1, 0))
    assert "hy_ev_native" in det and "hy_ev_action" not in det
    # The stepper with the event equations inside, with and without an action on the same events.
    oss = hy.model.nbody(6, masses=M, Gconst=G)
    V = {repr(s): s for s in oss.vars}
    kw = dict(high_accuracy=True, nt_events=[hy.nt_event(V["z_2"], hy.native_event_recorder())])
    act = hy.event_action({V[k]: (1.0 + 1e-9) * V[k] for k in ("vx_1", "vy_1", "vz_1")})
    a = hy.taylor_adaptive_batch(oss, None, 5, t_events=[hy.t_event(V["z_1"], callback=act)], **kw)
    c = hy.taylor_adaptive_batch(oss, None, 5, t_events=[hy.t_event(V["z_1"], callback=hy.native_event_counter())], **kw)
    assert "inside the stepper" in a.hip_source_mode and a.hip_source == c.hip_source
    assert a.event_log_code_object(0) == c.event_log_code_object(0) and a.event_log_code_object(1) == c.event_log_code_object(1)
    assert hy.hiprtc_compile(a.event_action_module()[0])[:4] == b"\x7fELF"


def _section(src, idx):
    body = src[src.index("hy_ev_action(const hy_eva_args a)"):]
    m = re.search(r"case %d: \{\n(.*?)break;\n\}" % idx, body, re.S)
    assert m, body
    return m.group(1).splitlines()


def test_the_swap_reads_both_operands_before_either_store():
    sys_, x, v = _osc(hy)
    ta = hy.taylor_adaptive_batch(sys_, None, 3, t_events=[hy.t_event(x, callback=hy.event_action({x: v, v: x}))])
    lines = _section(ta.event_action_module()[0], 0)
    loads = [k for k, ln in enumerate(lines) if re.search(r"= a\.state\[", ln)]
    stores = [k for k, ln in enumerate(lines) if re.match(r"a\.state\[.*\] = ", ln)]
    assert len(loads) == 2 and len(stores) == 2 and max(loads) < min(stores), lines
    # Row 0 receives what was read from row 1 and the other way round.
    name = {int(re.search(r"\(u64\)(\d+)u", lines[k]).group(1)): re.match(r"const double (\w+) =", lines[k]).group(1) for k in loads}
    res = dict(re.match(r"const double (r\d+) = (\w+);", ln).groups() for ln in lines if re.match(r"const double r\d+ = ", ln))
    got = {int(re.search(r"\(u64\)(\d+)u", lines[k]).group(1)): res[re.search(r"= (\w+);", lines[k]).group(1)] for k in stores}
    assert got == {0: name[1], 1: name[0]}, lines
    # Two actions on two events: two sections, each under the index of its event; an event without an action has none.
    tb = _bouncer(extra_t=[hy.t_event(x - 2.0, callback=hy.native_event_counter()), hy.t_event(v, callback=hy.event_action({x: x + 0.25}))])
    src = tb.event_action_module()[0]
    assert tb.n_event_actions == 2 and "case 0: {" in src and "case 2: {" in src and "case 1: {" not in src


EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_event_action")


def _build_cpp():
    """tests/cpp/test_event_action.cpp, compiled the way tests/test_independent_events.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_event_action.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_event_action_host_half():
    """The tag type as kw::callback, the error messages, where the events are applied, the C ABI."""
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_cpp_event_action_on_gpu():
    """One bounce and more through <heyoka/heyoka.hpp>, compared with a lambda callback."""
    out = subprocess.run([_build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the bouncing oscillator
# ---------------------------------------------------------------------------------------------------------------------
N_POOL = 131
N_STEPS = 40
T_END = 50.0


def _pool(n=N_POOL):
    """Distinct amplitudes in [0.4, 2) and phases spread over the circle: the systems bounce at different moments."""
    k = np.arange(n)
    amp = 0.4 + 1.6 * ((k * 29) % N_POOL) / N_POOL
    ph = 2.0 * np.pi * ((k * 53) % N_POOL) / N_POOL
    return np.stack([amp * np.cos(ph), -amp * np.sin(ph)])


def _collect(ta, cooldowns=True):
    oc, mn, mx, ns = ta.propagate_res_arrays()
    thi, tlo = ta.dtime
    d = {"state": np.array(ta.state), "thi": thi, "tlo": tlo, "outcome": np.asarray(oc, dtype=np.int64),
         "steps": np.asarray(ns, dtype=np.int64), "min_h": np.asarray(mn), "max_h": np.asarray(mx)}
    if cooldowns:
        cds = ta.te_cooldowns
        d["cd"] = np.array([[(-1.0, -1.0) if c is None else c for c in row] for row in cds]).reshape(ta.batch_size, -1)
    return d


def _same(a, b, cols_a=None, cols_b=None, what=""):
    """Bit for bit, key by key; cols_*: the systems to compare (default all)."""
    for k in a:
        if k not in b:
            continue
        x = a[k][..., cols_a] if (cols_a is not None and k == "state") else (a[k][cols_a] if cols_a is not None else a[k])
        y = b[k][..., cols_b] if (cols_b is not None and k == "state") else (b[k][cols_b] if cols_b is not None else b[k])
        assert np.array_equal(x, y, equal_nan=True), (what, k, x, y)


def _run(ta, n_steps=N_STEPS, t_end=T_END, between=None):
    """n_steps lock-step steps (outcomes, step sizes and states of every step), then propagate_until()."""
    per_step = []
    for _ in range(n_steps):
        ta.step()
        sr = ta.step_res
        per_step.append({"oc": np.array([int(o) for o, _ in sr]), "h": np.array([h for _, h in sr]), "state": np.array(ta.state)})
    after_steps = _collect(ta)
    if between is not None:
        between()
    ta.propagate_until(t_end)
    return per_step, after_steps, _collect(ta)


@functools.lru_cache(maxsize=None)
def _bounce_oracle(n):
    """The CPU oracle on the first n systems of the pool, its terminal callback doing the same multiplication."""
    _, ox, ov = _osc(ho)
    calls = []

    def cb(o, d_sgn, i):
        o.state.reshape(2, n)[1, i] *= BOUNCE
        calls.append(i)
        return True

    o = ho.OracleEventIntegrator(_osc(ho)[0], _pool()[:, :n], n, t_events=[ho.t_event(ox, cb, direction=NEG_HO)])
    per_step = []
    for _ in range(N_STEPS):
        res = o.step()
        per_step.append({"oc": np.array([r[0] for r in res]), "state": o.state.reshape(2, n).copy()})
    n_step_calls = len(calls)
    pr = o.propagate_until(T_END)
    return {"per_step": per_step, "n_step_calls": n_step_calls, "n_calls": len(calls), "state": o.state.reshape(2, n).copy(),
            "outcome": np.array([r[0] for r in pr]), "time": o.time_hi.copy()}


@pytest.mark.gpu
@pytest.mark.parametrize("emitter", [None, "table"])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_bouncing_oscillator(emitter, n):
    """The action on the device against the Python callback (bit for bit) and against the oracle."""
    st = _pool()[:, :n]
    n_py = [0]

    def py_cb(ta, d_sgn, i):
        ta.state_data()[1, i] *= BOUNCE
        n_py[0] += 1
        return True

    ta = _bouncer(n, state=st, emitter=emitter)
    tw = _bouncer(n, cb=py_cb, state=st, emitter=emitter)
    assert ta.event_stats["events_on_device"] is True and tw.event_stats["events_on_device"] is False
    assert ("table" in ta.hip_source_mode) == (emitter == "table"), ta.hip_source_mode
    n_py_at = []
    got, twin = _run(ta), _run(tw, between=lambda: n_py_at.append(n_py[0]))
    n_py_steps = n_py_at[0]
    for k in range(N_STEPS):
        _same(got[0][k], twin[0][k], what="step %d" % k)
    _same(got[1], twin[1], what="after the steps")
    _same(got[2], twin[2], what="after propagate_until")
    # The oracle: outcomes and event counts exactly, states within the tolerance of the event parity tests.
    ref = _bounce_oracle(n)
    n_fired = 0
    for k in range(N_STEPS):
        assert np.array_equal(got[0][k]["oc"], ref["per_step"][k]["oc"]), (k, got[0][k]["oc"], ref["per_step"][k]["oc"])
        n_fired += int(np.sum(got[0][k]["oc"] == 0))
        err = rel_err(got[0][k]["state"], ref["per_step"][k]["state"])
        print("step %d: rel_err vs oracle %.3g" % (k, err))
        assert err <= STATE_TOL, (k, err)
    # (A bounce every pi; a step of this system covers about 1: forty steps hold a good six bounces per system.)
    assert n_fired == n_py_steps == ref["n_step_calls"] and n_fired >= 5 * n
    assert np.array_equal(got[2]["outcome"], ref["outcome"]) and np.all(got[2]["outcome"] == int(OC.time_limit))
    assert n_py[0] == ref["n_calls"] and n_py[0] > n_py_steps
    err = rel_err(got[2]["state"], ref["state"])
    print("after propagate_until: rel_err vs oracle %.3g" % err)
    assert err <= STATE_TOL and np.array_equal(got[2]["thi"], ref["time"])
    # The bounce keeps every system on the side x >= 0 (up to the root finder's error at the bounce).
    assert np.all(got[2]["state"][0] >= -1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the yardstick - hy.cfunc of the same expressions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_multi_operation_action_equals_cfunc_on_the_device():
    """{x: x + par[0] sin(v), v: v cos(x) - time}: the assigned rows are, bit for bit, cfunc of the right-hand sides on the
    state before the action (a twin integrator whose callback is a counter), the parameters and time_hi; a system which did
    not fire keeps the twin's rows."""
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.par[0] * x)]
    rhs = [x + hy.par[0] * hy.sin(v), v * hy.cos(x) - hy.time]
    # Systems 0 and 2 reach x = 0 within the first step (x0 / |v0| = 0.1, 0.05), system 1 does not (x = 1.5 cos t).
    st = np.array([[0.1, 1.5, 0.07], [-1.0, 0.0, -1.4]])
    pars = np.array([[1.0, 1.3, 0.8]])
    t0 = np.array([0.25, 0.5, 3.0])
    kw = dict(pars=pars, time=t0)

    def build(cb):
        return hy.taylor_adaptive_batch(sys_, st, 3, t_events=[hy.t_event(x, callback=cb, direction=NEG_HY)], **kw)

    ctr = hy.native_event_counter()
    ta, tw = build(hy.event_action(list(zip([x, v], rhs)))), build(ctr)
    assert ta.event_stats["events_on_device"] is True and tw.event_stats["events_on_device"] is True
    ta.step()
    tw.step()
    oc = [int(o) for o, _ in ta.step_res]
    assert oc == [int(o) for o, _ in tw.step_res] and oc[0] == 0 and oc[2] == 0 and oc[1] == int(OC.success) and ctr.value == 2
    assert np.array_equal(ta.dtime[0], tw.dtime[0]) and np.array_equal(ta.dtime[1], tw.dtime[1])
    pre, post = np.array(tw.state), np.array(ta.state)
    want = hy.cfunc(rhs, [x, v])(pre, pars=pars, time=tw.dtime[0])
    assert np.array_equal(post[:, [0, 2]], want[:, [0, 2]]), (post, want)
    assert np.array_equal(post[:, 1], pre[:, 1])
    # (The action did something: the comparison above is not one of untouched rows.)
    assert np.all(post[:, [0, 2]] != pre[:, [0, 2]])
    # Cooldowns, Taylor coefficients and last_h are those of the truncated step.
    assert ta.te_cooldowns == tw.te_cooldowns and ta.te_cooldowns[0][0] is not None and ta.te_cooldowns[1][0] is None
    assert np.array_equal(ta.last_h, tw.last_h) and np.array_equal(ta.tc, tw.tc)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: first terminal event only
# ---------------------------------------------------------------------------------------------------------------------
# Chosen with the CPU oracle: amplitudes (0.7, 1.3, 0.9, 1.6, 1.1), phases (0.9, 4.1, 2.9, 5.2, 0.3). With the events
# x = 0 -> {v: -0.8 v}, x + 0.05 = 0 -> {x: x + 0.25} and v = 0.3 -> a counter (any direction), the oracle detects BOTH of
# the first two events inside one step at (step, system) = (0, 0): x = 0 first; (0, 1): x = -0.05 first; (2, 2): x = -0.05
# first; (2, 3): x = 0 first - and at nine more places within the first ten steps.
TWO_EVENT_STATE = np.array([[0.4351269777894651, -0.74727113049325, -0.8738623486346315, 0.7496266740806035, 1.0508701380381666],
                            [-0.5483288367392384, 1.0637602443837333, -0.21532439629258418, 1.4135274491522452, -0.32507222732747354]])
TWO_IN_ONE_STEP = {(0, 0): 0, (0, 1): 1, (2, 2): 1, (2, 3): 0}  # (step, system) -> index of the earlier event


def _two_event_kw(m, n, calls):
    _, x, v = _osc(m)
    if m is ho:
        def a0(o, d_sgn, i):
            o.state.reshape(2, n)[1, i] *= BOUNCE
            calls.append((i, 0))
            return True

        def a1(o, d_sgn, i):
            s = o.state.reshape(2, n)
            s[0, i] = s[0, i] + 0.25
            calls.append((i, 1))
            return True

        def a2(o, d_sgn, i):
            calls.append((i, 2))
            return True
        return [m.t_event(x, a0), m.t_event(x + 0.05, a1), m.t_event(v - 0.3, a2)]
    return [m.t_event(x, callback=hy.event_action({v: BOUNCE * v})), m.t_event(x + 0.05, callback=hy.event_action({x: x + 0.25})),
            m.t_event(v - 0.3, callback=calls)]


@pytest.mark.gpu
def test_only_the_first_terminal_event_of_a_step_acts(monkeypatch):
    n = 5
    detected = {}
    cur = {"step": 0, "sys": 0}
    orig = ho.detect_events

    def spy(tc, h, g_eps, evs, terminal, cds, p):
        r = orig(tc, h, g_eps, evs, terminal, cds, p)
        if terminal:
            detected[(cur["step"], cur["sys"])] = sorted((abs(e[1]), e[0]) for e in r)
            cur["sys"] += 1
        return r

    monkeypatch.setattr(ho, "detect_events", spy)
    calls_o = []
    o = ho.OracleEventIntegrator(_osc(ho)[0], TWO_EVENT_STATE, n, t_events=_two_event_kw(ho, n, calls_o))
    ctr = hy.native_event_counter()
    ta = hy.taylor_adaptive_batch(_osc(hy)[0], TWO_EVENT_STATE, n, t_events=_two_event_kw(hy, n, ctr))
    assert ta.event_stats["events_on_device"] is True and ta.n_event_actions == 2
    n_act = [0, 0, 0]
    for k in range(10):
        cur["step"], cur["sys"] = k, 0
        res = o.step()
        ta.step()
        oc = np.array([int(c) for c, _ in ta.step_res])
        assert np.array_equal(oc, np.array([r[0] for r in res])), (k, oc, res)
        for e in range(3):
            n_act[e] += int(np.sum(oc == e))
        err = rel_err(ta.state, o.state.reshape(2, n))
        print("step %d: outcomes %s rel_err vs oracle %.3g" % (k, oc.tolist(), err))
        # (An action applied for the later event as well would be off by 0.25 in x, or by 1.8 |v| in v.)
        assert err <= STATE_TOL, (k, err)
        for (kk, i), first in TWO_IN_ONE_STEP.items():
            if kk == k:
                ev = [e for _, e in detected[(k, i)]]
                assert ev[:2] == [first, 1 - first], (k, i, detected[(k, i)])
                assert oc[i] == first
    assert n_act == [sum(1 for _, e in calls_o if e == q) for q in range(3)] and n_act[0] > 0 and n_act[1] > 0 and n_act[2] > 0
    assert ctr.value == n_act[2]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: outer Solar System, the event equations inside the one-lane-per-pair stepper
# ---------------------------------------------------------------------------------------------------------------------
KICK = 1.0 + 1e-9
OSS_T = 12.0  # Jupiter crosses the plane z = 0 every 5.93 years: every system at least once


@functools.lru_cache(maxsize=None)
def _oss_pool(n):
    """Lane j of configs.outer_ss_state propagated by 3 j years by an event-free integrator (spread phases, the systems of
    tests/test_independent_events.py); for n > 9 the phases repeat every 9 systems on perturbed initial conditions."""
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    pre = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), configs.outer_ss_state(n, perturb=1e-3, seed=14), n,
                                   high_accuracy=True)
    pre.propagate_until(3.0 * (np.arange(n) % 9))
    st = np.array(pre.state)
    st.setflags(write=False)
    return st


def _oss(st, cb="action", **kw):
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    oss = hy.model.nbody(6, masses=M, Gconst=G)
    V = {repr(s): s for s in oss.vars}
    n = st.shape[1]
    if cb == "action":
        cb = hy.event_action({V[k]: KICK * V[k] for k in ("vx_1", "vy_1", "vz_1")})
    ta = hy.taylor_adaptive_batch(oss, st, n, high_accuracy=True, t_events=[hy.t_event(V["z_1"], callback=cb)],
                                  nt_events=[hy.nt_event(V["z_2"], hy.native_event_recorder())], **kw)
    assert "v5" in ta.hip_source_mode and "inside the stepper" in ta.hip_source_mode, ta.hip_source_mode
    return ta


@pytest.mark.gpu
def test_outer_solar_system_kick_at_the_plane_crossing():
    n = 5
    st = _oss_pool(n)
    fired = []

    def py_cb(ta, d_sgn, i):
        sd = ta.state_data()
        for r in (9, 10, 11):
            sd[r, i] *= KICK
        fired.append(i)
        return True

    ta, tw = _oss(st), _oss(st, cb=py_cb)
    assert ta.event_stats["events_on_device"] is True and tw.event_stats["events_on_device"] is False
    for _ in range(6):
        ta.step()
        tw.step()
        assert [int(o) for o, _ in ta.step_res] == [int(o) for o, _ in tw.step_res]
        assert np.array_equal(ta.state, tw.state)
    ta.propagate_until(OSS_T)
    tw.propagate_until(OSS_T)
    _same(_collect(ta), _collect(tw))
    assert sorted(set(fired)) == list(range(n)) and len(fired) >= n
    # The rows of the event log (Saturn's crossings, states included) are the same rows.
    la, lt = ta.event_log, tw.event_log
    assert len(la) == len(lt) and np.array_equal(la.rows, lt.rows)
    assert len(la) >= 1 and np.all(la.terminal == False) and np.max(np.abs(la.state[:, 14])) <= 1e-12  # noqa: E712


# ---------------------------------------------------------------------------------------------------------------------
# GPU: host-loop path of a mixed integrator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_integrator_applies_the_action_in_the_host_loop():
    """The action next to a Python non-terminal callback: the host loop applies it through the same compiled section - the
    bits of the device path on the same event equations (which take part in the step-size selection: the device-path
    integrator carries the non-terminal event with a counter), and the later callbacks of the step see the changed state."""
    n = 3
    st = _pool()[:, :n]
    _, x, v = _osc(hy)
    seen = []
    ctr = hy.native_event_counter()
    dev = _bouncer(n, state=st, nt=[hy.nt_event(v - 0.2, ctr)])
    mix = _bouncer(n, state=st, nt=[hy.nt_event(v - 0.2, lambda ta, t, d, i: seen.append((i, t)))])
    assert dev.event_stats["events_on_device"] is True and mix.event_stats["events_on_device"] is False
    a, b = _run(dev), _run(mix)
    for k in range(N_STEPS):
        _same(a[0][k], b[0][k], what="step %d" % k)
    _same(a[1], b[1], what="after the steps")
    _same(a[2], b[2], what="after propagate_until")
    assert len(seen) == ctr.value > 0 and sum(int(np.sum(s["oc"] == 0)) for s in a[0]) >= 5 * n
    # Callbacks which run later in the step see the changed state: two systems start at the same point and bounce in the
    # same (first) step, x = 0.3 - t + ...; the non-terminal event x = 0.01 of system 1 fires just before its own bounce and
    # its callback runs after the action of system 0.
    st2 = np.array([[0.3, 0.3], [-1.0, -1.0]])
    views = []

    def look(ta, t, d_sgn, i):
        if i == 1:
            views.append(np.array(ta.state))

    mix2 = _bouncer(2, state=st2, nt=[hy.nt_event(x - 0.01, look, direction=NEG_HY)])
    mix2.step()
    assert [int(o) for o, _ in mix2.step_res] == [0, 0] and len(views) == 1
    after = np.array(mix2.state)
    assert np.array_equal(views[0][:, 0], after[:, 0]) and after[1, 0] > 0.8 and views[0][1, 1] < -1.0
    assert np.array_equal(after[:, 0], after[:, 1])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: independent semantics
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_independent_semantics_a_bounce_does_not_retire():
    """A plain stop (x = 1, upwards) next to the action, 9 systems starting at phase 1.2 with the amplitudes A below: the
    bounce leaves the amplitude 0.8 A, so the systems with 0.8 A > 1 rise through x = 1 after their first bounce and are
    retired there, the others bounce until the end. System i equals the system alone in a batch of 1 under the default
    semantics (the yardstick of tests/test_independent_events.py)."""
    amps = np.array([0.6, 1.5, 0.9, 2.0, 1.1, 1.3, 0.7, 1.8, 1.0])
    n, t_end = len(amps), 20.0
    st = np.stack([amps * np.cos(1.2), -amps * np.sin(1.2)])
    _, x, v = _osc(hy)
    stop = [hy.t_event(x - 1.0, direction=POS_HY)]
    ta = _bouncer(n, state=st, extra_t=stop, batch_semantics="independent")
    assert ta.event_stats["events_on_device"] is True
    ta.propagate_until(t_end)
    got = _collect(ta)
    retire = 0.8 * amps > 1.0
    assert np.array_equal(got["outcome"], np.where(retire, -2, int(OC.time_limit))), got["outcome"]
    assert ta.n_retired == int(np.sum(retire)) == 4
    assert np.all(got["thi"][~retire] == t_end) and np.all(got["thi"][retire] < 4.0)
    assert np.max(np.abs(got["state"][0, retire] - 1.0)) <= 1e-13
    solo = _bouncer(1, state=st[:, :1], extra_t=stop)
    assert solo.event_stats["events_on_device"] is False
    for i in range(n):
        solo.state = st[:, i:i + 1]
        solo.dtime = ([0.0], [0.0])
        solo.reset_cooldowns()
        solo.propagate_until(t_end)
        _same(got, _collect(solo), cols_a=slice(i, i + 1), what="system %d" % i)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: batch-size independence
# ---------------------------------------------------------------------------------------------------------------------
def _windows(S, n_pool):
    """(first system, size): prefixes of 1, 2, 3, S + 1 and 65 systems and a window which starts at system 5."""
    return list(dict.fromkeys([(0, 1), (0, 2), (0, 3), (0, S + 1), (0, 65), (5, 3)]))


@pytest.mark.gpu
def test_batch_size_independence_straight_line_stepper():
    pool = _pool()
    tf = T_END * (0.5 + ((np.arange(N_POOL) * 17) % N_POOL) / N_POOL)

    def run(first, size):
        ta = _bouncer(size, state=pool[:, first:first + size])
        assert "lanes per system: 1," in ta.hip_source_mode and ta.event_stats["events_on_device"] is True
        for _ in range(10):
            ta.step()
        mid = _collect(ta)
        ta.propagate_until(tf[first:first + size] if size > 1 else float(tf[first]))
        return mid, _collect(ta)

    ref = run(0, N_POOL)
    assert np.all(ref[1]["outcome"] == int(OC.time_limit))
    for first, size in _windows(64, N_POOL):
        got = run(first, size)
        for a, b in zip(got, ref):
            _same(a, b, cols_b=slice(first, first + size), what="window (%d, %d)" % (first, size))


@pytest.mark.gpu
def test_batch_size_independence_one_lane_per_pair_stepper():
    pool = _oss_pool(N_POOL)

    def run(first, size):
        ta = _oss(pool[:, first:first + size])
        assert "lanes per system: 16" in ta.hip_source_mode and ta.event_stats["events_on_device"] is True
        ta.propagate_until(OSS_T)
        d = _collect(ta)
        log = ta.event_log
        d["log"] = [log.rows[log.system == i][:, 1:] for i in range(size)]
        return d

    ref = run(0, N_POOL)
    assert np.all(ref["outcome"] == int(OC.time_limit))
    # (Every system was kicked: its cooldown is running or it has been through one; the states differ from an integration
    # without the action - checked against the twin in test_outer_solar_system_kick_at_the_plane_crossing.)
    for first, size in _windows(4, N_POOL):
        got = run(first, size)
        logs_a, logs_b = got.pop("log"), ref["log"][first:first + size]
        _same(got, {k: v for k, v in ref.items() if k != "log"}, cols_b=slice(first, first + size), what="window (%d, %d)" % (first, size))
        for a, b in zip(logs_a, logs_b):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: copies made by the ensemble driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ensemble_copies_keep_the_action():
    n, t_end = 3, 20.0
    st = _pool()[:, :n]

    def gen(ta_copy, i):
        ta_copy.state = st * (1.0 + 0.5 * i)

    base = _bouncer(n, state=st)
    outs = hy.ensemble_propagate_until_batch(base, t_end, 2, gen, n_devices=1)
    assert len(outs) == 2
    for i, out in enumerate(outs):
        serial = _bouncer(n, state=st * (1.0 + 0.5 * i))
        serial.propagate_until(t_end)
        assert out.n_event_actions == 1 and out.event_stats["events_on_device"] is True
        _same(_collect(out, cooldowns=False), _collect(serial, cooldowns=False), what="iteration %d" % i)
        # (Bounced: never below x = 0, and not the free oscillation.)
        assert np.all(out.state[0] >= -1e-12)
    free = hy.taylor_adaptive_batch(_osc(hy)[0], st, n)
    free.propagate_until(t_end)
    assert not np.array_equal(free.state, outs[0].state)
