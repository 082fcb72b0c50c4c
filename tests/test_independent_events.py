"""batch_semantics = "independent": within one propagate_until() / propagate_for() / propagate_grid() call a system whose
step ends in a stopping terminal event (or in a non-finite state) is retired ALONE - sticky outcome, zero-length steps -
while the other systems carry on; terminal events without a callback are applied on the device.

The yardstick is the system run alone. Every kernel family with events is held to batch-size independence bit for bit
(tests/test_batch_independence.py), so under the new semantics system i of a batch must equal, bit for bit, the same
system run in a batch of 1 under the DEFAULT semantics (where the first stopping event ends the call): state, time
(hi, lo), outcome, step count, min / max |h|, cooldowns, its grid rows (NaN pattern included) and its rows of the event
log (column 0, the system, aside). The solo runs and the batches are also held to OracleEventIntegrator(batch_size=1):
outcomes and step counts exactly, states / times / step sizes within the tolerances of the family's event tests in
tests/test_gpu_parity.py (small systems: state 1e5 eps, time 1e-13, step sizes 1e6 eps; outer Solar System on the
wave-cluster steppers: state 1e7 eps per row after a propagation, time 1e-10, step sizes 1e6 eps).

Every scenario is chosen with the oracle on the CPU so that the oracle alone shows: at least a quarter of the systems
retire, at least a quarter reach their final time, and a surviving system takes at least 3 more steps after the first
retirement (_honest())."""
import ctypes
import functools
import os
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
RETIRED_BY_EVENT = -1  # -index - 1 of terminal event 0


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def _osc(m):
    if m is ho:
        x, v = ho.var("x"), ho.var("v")
        return [(x, v), (v, -1.0 * x)], x, v
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -x)], x, v


def _plain_stop(batch_semantics=None, n=3, **kw):
    sys_, x, v = _osc(hy)
    return hy.taylor_adaptive_batch(sys_, None, n, batch_semantics=batch_semantics,
                                    t_events=[hy.t_event(x - 1.0, direction=NEG_HY)], **kw)


def test_the_new_value_is_accepted_without_a_gpu_and_others_are_rejected():
    ta = _plain_stop("independent")
    assert ta.with_events and ta.n_retired == 0
    lib = _lib.lib
    # hy_tab_config of the C ABI, as ctypes sees it.
    sys_ = ta._sys
    for value in (0, 1, 2, 3):
        cfg = _lib.TabConfig()
        cfg.batch_semantics = value
        h = lib.hy_tab_create(sys_._h, None, 0, 4, ctypes.byref(cfg))
        assert h, _lib.last_error()
        assert lib.hy_tab_get_n_retired(h) == 0
        lib.hy_tab_free(h)
    for value in (4, 7, -1):
        cfg = _lib.TabConfig()
        cfg.batch_semantics = value
        h = lib.hy_tab_create(sys_._h, None, 0, 4, ctypes.byref(cfg))
        assert not h
        msg = _lib.last_error()
        assert msg.startswith("Invalid batch semantics") and "3 independent" in msg and "0 reference" in msg, msg
    with pytest.raises(ValueError, match="batch_semantics"):
        _plain_stop("retire")


EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_independent_events")


def _build_cpp():
    """tests/cpp/test_independent_events.cpp, compiled the way tests/test_event_recorder.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_independent_events.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_independent_events_host_half():
    """kw::batch_semantics = 3 and hy_tab_config::batch_semantics = 3 are accepted, 4 and 7 rejected with the stated prefix."""
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_cpp_independent_events_on_gpu():
    out = subprocess.run([_build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


def test_the_sources_are_the_same_text_for_every_semantics():
    """The stop flags and the sticky outcomes are data, not code: stepper source, event-log code objects and the
    event-detection source do not depend on the semantics."""
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    oss = hy.model.nbody(6, masses=M, Gconst=G)
    x1, x2 = hy.make_vars("x_1", "x_2")
    sys_, x, v = _osc(hy)

    def variants(sem):
        return [
            _plain_stop(sem),
            _plain_stop(sem, emitter="table"),
            hy.taylor_adaptive_batch(sys_, None, 3, batch_semantics=sem, nt_events=[hy.nt_event(v, hy.native_event_recorder())],
                                     t_events=[hy.t_event(x - 1.0, direction=NEG_HY)]),
            hy.taylor_adaptive_batch(oss, None, 8, high_accuracy=True, batch_semantics=sem,
                                     t_events=[hy.t_event(x1 - x2, hy.native_event_recorder())]),
        ]

    ref = variants(None)
    assert "inside the stepper" in ref[3].hip_source_mode
    for sem in ("lockstep", "per_lane", "independent"):
        for a, b in zip(ref, variants(sem)):
            assert a.hip_source == b.hip_source and a.hip_source_mode == b.hip_source_mode
            assert a.code_object == b.code_object
    for a, b in zip(ref[2:], variants("independent")[2:]):
        for which in (0, 1):
            assert a.event_log_code_object(which) == b.event_log_code_object(which)
    # (The event-detection source is a function of (order, events) alone: hy_event_detection_source() has no semantics
    # argument, and tests/test_event_recorder.py pins its text by hash.)
    src = _lib.take_str(_lib.lib.hy_event_detection_source(20, 1, 1))
    assert "hy_ev_native" in src and "te_stop" not in src and "hy_ev_stop" not in src


def test_where_the_events_are_applied_is_unchanged_for_the_other_semantics():
    """event_stats["events_on_device"]: counters and recorders always; a terminal event without a callback only under the
    new semantics; any caller callback keeps the host loop."""
    sys_, x, v = _osc(hy)
    for sem, plain in ((None, False), ("reference", False), ("lockstep", False), ("per_lane", False), ("independent", True)):
        assert _plain_stop(sem).event_stats["events_on_device"] is plain
        mk = functools.partial(hy.taylor_adaptive_batch, sys_, None, 3, batch_semantics=sem)
        native = mk(nt_events=[hy.nt_event(v, hy.native_event_recorder())], t_events=[hy.t_event(x - 1.0, hy.native_event_counter())])
        assert native.event_stats["events_on_device"] is True
        with_stop = mk(nt_events=[hy.nt_event(v, hy.native_event_counter())], t_events=[hy.t_event(x - 1.0, direction=NEG_HY)])
        assert with_stop.event_stats["events_on_device"] is plain
        mixed = mk(nt_events=[hy.nt_event(v, lambda *a: None)], t_events=[hy.t_event(x - 1.0, direction=NEG_HY)])
        assert mixed.event_stats["events_on_device"] is False
        assert mk().event_stats["events_on_device"] is False


# ---------------------------------------------------------------------------------------------------------------------
# GPU: scenarios
# ---------------------------------------------------------------------------------------------------------------------
def _amplitudes(n):
    """Alternating below / above 1: 0.5, 1.1, 0.9, 1.5, 3, ... The systems with A > 1 stop at acos(1 / A)."""
    a = [0.5, 1.1, 0.9, 1.5, 3.0]
    for i in range(5, n):
        a.append(0.3 + 0.6 * ((i * 7) % 11) / 11.0 if i % 2 == 0 else 1.1 + 2.0 * ((i * 5) % 13) / 13.0)
    return np.array(a[:n])


# Distance of the CPU oracle's event times from the closed form acos(1 / A), maximum over _amplitudes(65), measured when
# the test was written (tests: test_oscillator_*; the oracle is re-measured there and must not exceed it).
ORACLE_EVENT_TIME_ERR = 2.220446049250313e-16
EVENT_TIME_BOUND = 10 * ORACLE_EVENT_TIME_ERR


class Scenario:
    """A system, its events for either library, the initial states of S systems and their final times."""

    def __init__(self, name, states, tf, kw=None, ho_kw=None, host_cb=False, state_tol=1e5 * EPS, time_tol=1e-13, rows=False):
        self.name, self.states, self.tf = name, np.asarray(states, dtype=float), np.asarray(tf, dtype=float)
        self.kw, self.ho_kw, self.host_cb = dict(kw or {}), dict(ho_kw or {}), host_cb
        self.state_tol, self.time_tol, self.rows = state_tol, time_tol, rows

    def system(self, m):
        raise NotImplementedError

    def events(self, m, off):
        """Keyword arguments t_events / nt_events. off: the index of the first system of the batch in the scenario (a
        callback which looks at the batch index sees the system's own number in a solo run)."""
        raise NotImplementedError


class Oscillator(Scenario):
    def system(self, m):
        return _osc(m)[0]

    def events(self, m, off):
        _, x, v = _osc(m)
        neg = NEG_HO if m is ho else NEG_HY
        if not self.host_cb:
            return {"t_events": [m.t_event(x - 1.0, direction=neg)]}
        # Host-callback path: the terminal callback lets the even systems pass; a recorder on the non-terminal event v.
        cb = (lambda ta, d_sgn, i: (off + i) % 2 == 0)
        # (The oracle counts the invocations per system: the rows the log must hold.)
        seen = self.nt_seen = getattr(self, "nt_seen", {})
        rec = (lambda ta, t, d_sgn, i: seen.__setitem__(off + i, seen.get(off + i, 0) + 1)) if m is ho else hy.native_event_recorder()
        return {"t_events": [m.t_event(x - 1.0, cb, direction=neg)], "nt_events": [m.nt_event(v, rec)]}


class Blowup(Scenario):
    """x' = x^2, v' = -v: a system with x(0) > 0 goes non-finite; the terminal event v = 0.2 (no callback) retires others."""

    def system(self, m):
        if m is ho:
            x, v = ho.var("x"), ho.var("v")
            return [(x, x * x), (v, -1.0 * v)]
        x, v = hy.make_vars("x", "v")
        return [(x, x * x), (v, -v)]

    def events(self, m, off):
        v = ho.var("v") if m is ho else hy.make_vars("v", "dummy__")[0]
        return {"t_events": [m.t_event(v - 0.2, direction=NEG_HO if m is ho else NEG_HY)]}


class OuterSS(Scenario):
    def system(self, m):
        return m.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G) if m is ho else hy.model.nbody(
            6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)

    def events(self, m, off):
        mk = (lambda s_: m.var(s_)) if m is ho else (lambda s_: m.make_vars(s_, "dummy__")[0])
        x1, y1, z1, x2, y2, z2 = [mk(s_) for s_ in ("x_1", "y_1", "z_1", "x_2", "y_2", "z_2")]
        d2 = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2) - 81.0
        return {"t_events": [m.t_event(d2, direction=NEG_HO if m is ho else NEG_HY)]}


def _collect(ta):
    """What is compared of every system of an integrator after a call (one download of each array)."""
    oc, mn, mx, ns = ta.propagate_res_arrays()
    thi, tlo = ta.dtime
    st, cds = np.array(ta.state), ta.te_cooldowns
    rows = ta.event_log.rows if ta.event_log_size else None
    out = []
    for i in range(ta.batch_size):
        d = {"state": st[:, i].copy(), "time": (float(thi[i]), float(tlo[i])), "outcome": int(oc[i]), "steps": int(ns[i]),
             "min_h": float(mn[i]), "max_h": float(mx[i]), "cd": cds[i]}
        # (Rows of the event log of the system, without column 0 - the system.)
        d["log"] = np.zeros((0, 0)) if rows is None else np.array(rows[rows[:, 0] == i][:, 1:])
        out.append(d)
    return out


def _same(a, b):
    assert a["outcome"] == b["outcome"] and a["steps"] == b["steps"], (a, b)
    if a["outcome"] == int(OC.err_nf_state):
        return  # (retired as non-finite: only the outcome and the step count are specified)
    for k in ("state",):
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])
    for k in ("time", "outcome", "steps", "cd"):
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("min_h", "max_h"):
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])
    assert a["log"].size == b["log"].size and np.array_equal(a["log"].reshape(-1), b["log"].reshape(-1)), (a["log"], b["log"])


class _Solo:
    """One batch-1 integrator per scenario under the default semantics; state, time, cooldowns and the log are reset
    between systems."""

    def __init__(self, sc):
        self.sc = sc
        # (The callback of the host-callback scenario closes over the offset: rebuilt per system through a mutable cell.)
        self.cell = cell = {"off": 0}
        if sc.host_cb:
            _, x, v = _osc(hy)
            ev = {"t_events": [hy.t_event(x - 1.0, lambda ta, d_sgn, i: (cell["off"] + i) % 2 == 0, direction=NEG_HY)],
                  "nt_events": [hy.nt_event(v, hy.native_event_recorder())]}
        else:
            ev = sc.events(hy, 0)
        self.ta = hy.taylor_adaptive_batch(sc.system(hy), sc.states[:, :1], 1, **ev, **sc.kw)

    def run(self, j, calls):
        ta = self.ta
        self.cell["off"] = j
        ta.state = self.sc.states[:, j:j + 1]
        ta.dtime = ([0.0], [0.0])
        ta.reset_cooldowns()
        if ta.event_log_size:
            ta.clear_event_log()
        out = []
        for call in calls:
            call(ta, np.array([j]))
            out.append(_collect(ta)[0])
        return out


@functools.lru_cache(maxsize=None)
def _solo(sc):
    return _Solo(sc)


def _oracle(sc, j, calls_o):
    """The oracle's run of system j alone: list of (outcome, steps, min_h, max_h, state, time) per call."""
    o = ho.OracleEventIntegrator(sc.system(ho), sc.states[:, j], 1, **sc.events(ho, j), **sc.ho_kw)
    out = []
    for call in calls_o:
        pr = call(o, j)
        out.append({"outcome": int(pr[0][0]), "steps": int(pr[0][3]), "min_h": pr[0][1], "max_h": pr[0][2],
                    "state": o.state.copy(), "time": float(o.time_hi[0])})
    return out


def _honest(ref, n_calls=1):
    """The conditions which keep a test honest, on the ORACLE's results (list over systems of lists over calls)."""
    for c in range(n_calls):
        oc = np.array([r[c]["outcome"] for r in ref])
        steps = np.array([r[c]["steps"] for r in ref])
        retired = (oc == RETIRED_BY_EVENT) | (oc == int(OC.err_nf_state))
        done = oc == int(OC.time_limit)
        n = len(ref)
        assert 4 * np.sum(retired) >= n and 4 * np.sum(done) >= n, (oc,)
        # (A retired system has taken one step per sweep: its step count is the sweep which retired it. A non-finite step
        # is not counted: that sweep is the count plus one.)
        first = np.min(steps[retired] + (oc[retired] == int(OC.err_nf_state)))
        assert np.max(steps[~retired]) >= first + 3, (oc, steps)


def _vs_oracle(sc, got, ref):
    """Systems (list) against their oracle runs: outcomes and step counts exactly; states over the ensemble with the error
    measure of the family's tests in tests/test_gpu_parity.py - rel_err() for the small systems, the row-scaled
    row_rel_err() (scale: max |reference| of the state variable over the ensemble) for the outer Solar System."""
    assert [g["outcome"] for g in got] == [r["outcome"] for r in ref], ([g["outcome"] for g in got], [r["outcome"] for r in ref])
    assert [g["steps"] for g in got] == [r["steps"] for r in ref], ([g["steps"] for g in got], [r["steps"] for r in ref])
    # (A system retired as non-finite: only the outcome and the step count are specified.)
    ok = [k for k, r in enumerate(ref) if r["outcome"] != int(OC.err_nf_state)]
    a = np.stack([got[k]["state"] for k in ok], axis=1)
    b = np.stack([ref[k]["state"].reshape(-1) for k in ok], axis=1)
    if sc.rows:
        err = np.max(np.max(np.abs(a - b), axis=1) / (np.max(np.abs(b), axis=1) + 1e-300))
    else:
        err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    assert err <= sc.state_tol, err
    for k in ok:
        assert abs(got[k]["time"][0] - ref[k]["time"]) <= sc.time_tol, (got[k]["time"], ref[k]["time"])
        for q in ("min_h", "max_h"):
            if np.isfinite(ref[k][q]) and ref[k][q] != 0.0:
                assert abs(got[k][q] - ref[k][q]) <= 1e6 * EPS * abs(ref[k][q]), (q, got[k][q], ref[k][q])
            else:
                assert got[k][q] == ref[k][q], (q, got[k][q], ref[k][q])


def _run_batch(sc, idx, calls, **ctor):
    """Systems idx of the scenario in one integrator under the new semantics; per call the list of collected systems."""
    idx = np.asarray(idx)
    ta = hy.taylor_adaptive_batch(sc.system(hy), sc.states[:, idx], len(idx), batch_semantics="independent",
                                  **sc.events(hy, int(idx[0])), **sc.kw, **ctor)
    out = []
    for call in calls:
        call(ta, idx)
        res = _collect(ta)
        n_ret = sum(1 for r in res if r["outcome"] == RETIRED_BY_EVENT or r["outcome"] == int(OC.err_nf_state))
        assert ta.n_retired == n_ret, (ta.n_retired, [r["outcome"] for r in res])
        out.append(res)
    return ta, out


def _check(sc, idx, calls, calls_o, **ctor):
    """Batch (new semantics) == solo runs (default semantics) bit for bit; both against the oracle; honesty conditions."""
    idx = list(idx)
    ref = [_oracle(sc, j, calls_o) for j in idx]
    if len(idx) >= 3:
        _honest(ref, len(calls))
    ta, got = _run_batch(sc, idx, calls, **ctor)
    solo = _solo(sc)
    alone = [solo.run(j, calls) for j in idx]
    for c in range(len(calls)):
        for k in range(len(idx)):
            _same(got[c][k], alone[k][c])
        _vs_oracle(sc, [a[c] for a in alone], [r[c] for r in ref])
        _vs_oracle(sc, got[c], [r[c] for r in ref])
    return ta, got, ref


# ---------------------------------------------------------------------------------------------------------------------
# GPU: oscillator, plain stop (applied on the device)
# ---------------------------------------------------------------------------------------------------------------------
def _osc_scenario(emitter, host_cb=False, n=65, amps=None):
    a = _amplitudes(n) if amps is None else np.asarray(amps, dtype=float)
    return _OSC_CACHE.setdefault((emitter, host_cb, tuple(a)), Oscillator(
        "oscillator", np.stack([a, np.zeros(len(a))]), np.full(len(a), 10.0), kw=({"emitter": emitter} if emitter else {}), host_cb=host_cb))


_OSC_CACHE = {}
P_UNTIL = lambda tf, **kw: (lambda ta, idx: ta.propagate_until(tf[idx] if ta.batch_size > 1 else float(tf[idx[0]]), **kw))  # noqa: E731
O_UNTIL = lambda tf, **kw: (lambda o, j: o.propagate_until(float(tf[j]), **kw))  # noqa: E731


@pytest.mark.gpu
@pytest.mark.parametrize("emitter", [None, "table"])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_oscillator_plain_stop_on_the_device(emitter, n):
    sc = _osc_scenario(emitter)
    ta, got, ref = _check(sc, range(n), [P_UNTIL(sc.tf)], [O_UNTIL(sc.tf)])
    assert ta.event_stats["events_on_device"] is True
    assert ("table" in ta.hip_source_mode) == (emitter == "table"), ta.hip_source_mode
    amps = sc.states[0, :n]
    for a, g, r in zip(amps, got[0], ref):
        if a > 1.0:
            # Closed form: the oracle within the recorded distance, the integrator within ten times that.
            assert abs(r[0]["time"] - np.arccos(1.0 / a)) <= ORACLE_EVENT_TIME_ERR
            assert g["outcome"] == RETIRED_BY_EVENT and abs(g["time"][0] - np.arccos(1.0 / a)) <= EVENT_TIME_BOUND
            assert g["cd"][0] is not None and g["cd"][0][0] == 0.0
        else:
            assert g["outcome"] == int(OC.time_limit) and g["time"] == (10.0, 0.0)
    if n == 65:
        # The device outcome array reports the sticky outcomes, not the time_limit of the zero-length steps.
        import torch

        dev = torch.as_tensor(ta.device_array("outcome"), device="cuda").cpu().numpy()
        assert np.array_equal(dev, np.array([g["outcome"] for g in got[0]]))
        assert ta.n_retired == int(np.sum(amps > 1.0)) >= 32


# ---------------------------------------------------------------------------------------------------------------------
# GPU: outer Solar System, the event equations inside the one-lane-per-pair stepper / the one-system-per-lane steppers
# ---------------------------------------------------------------------------------------------------------------------
OSS_HORIZON = 10.0  # about half a synodic period of Jupiter and Saturn (19.86 yr); chosen with the oracle


@functools.lru_cache(maxsize=None)
def _oss_scenario(n, on_cluster):
    """Lane j of configs.outer_ss_state propagated by 3 j years by an event-free integrator (per-lane final times): the
    phases of the Jupiter - Saturn distance are spread, so that retired and surviving systems share wavefronts."""
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    pre = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), configs.outer_ss_state(n, perturb=1e-3, seed=14), n,
                                   high_accuracy=True)
    pre.propagate_until(3.0 * np.arange(n))
    return OuterSS("outer_ss", np.array(pre.state), np.full(n, OSS_HORIZON),
                   kw={"high_accuracy": True, **({} if on_cluster else {"events_on_cluster": False})}, ho_kw={"high_accuracy": True},
                   state_tol=1e7 * EPS, time_tol=1e-10, rows=True)


@pytest.mark.gpu
@pytest.mark.parametrize("on_cluster", [True, False])
@pytest.mark.parametrize("n", [5, 9])
def test_outer_solar_system_close_encounter_stop(n, on_cluster):
    sc = _oss_scenario(n, on_cluster)
    ta, got, _ = _check(sc, range(n), [P_UNTIL(sc.tf)], [O_UNTIL(sc.tf)])
    mode = ta.hip_source_mode
    if on_cluster:
        assert "v5" in mode and "inside the stepper" in mode, mode
    else:
        assert "inside the stepper" not in mode and not mode.startswith("cluster"), mode
    assert ta.event_stats["events_on_device"] is True
    for g in got[0]:
        if g["outcome"] == RETIRED_BY_EVENT:
            # (Jupiter - Saturn distance 9 AU at the retirement, and the system did not move afterwards.)
            d = g["state"][6:9] - g["state"][12:15]
            assert abs(np.dot(d, d) - 81.0) <= 1e-10 and g["time"][0] < OSS_HORIZON


# ---------------------------------------------------------------------------------------------------------------------
# GPU: host-callback path (mixed integrator: a caller callback and a recorder)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_callback_path_retires_the_odd_systems_and_keeps_the_log_rows():
    amps = 1.1 + 0.3 * np.arange(6)
    sc = _osc_scenario(None, host_cb=True, amps=amps)
    ta, got, _ = _check(sc, range(6), [P_UNTIL(sc.tf)], [O_UNTIL(sc.tf)])
    assert ta.event_stats["events_on_device"] is False
    for j, g in enumerate(got[0]):
        assert g["outcome"] == (RETIRED_BY_EVENT if j % 2 else int(OC.time_limit))
        # Rows of the recorder on v, as many as the oracle invoked its callback: the zero of v at t = 0 for every system,
        # and those at pi, 2 pi, 3 pi for the systems which pass through the event.
        assert g["log"].shape[0] == sc.nt_seen[j] == (1 if j % 2 else 4), (g["log"], sc.nt_seen)
        assert np.all(g["log"][:, 0] == 1.0) and np.max(np.abs(g["log"][:, 3] - np.pi * np.arange(g["log"].shape[0]))) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# GPU: propagate_grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_propagate_grid_rows_of_a_retired_system():
    sc = _osc_scenario(None, amps=_amplitudes(5))
    grid = np.linspace(0.0, 8.0, 9)
    outs = {}

    def call(ta, idx):
        outs[ta.batch_size, int(idx[0])] = np.array(ta.propagate_grid(grid)[1])

    def call_o(o, j):
        return o.propagate_until(8.0)

    ta, got, ref = _check(sc, range(5), [call], [call_o])
    out = outs[5, 0]
    first_retirement = min(r[0]["steps"] for r in ref if r[0]["outcome"] == RETIRED_BY_EVENT)
    for j in range(5):
        assert np.array_equal(out[:, :, j], outs[1, j][:, :, 0], equal_nan=True)
        t_end = got[0][j]["time"][0]
        reached = grid <= t_end
        assert np.all(np.isfinite(out[reached, :, j])) and np.all(np.isnan(out[~reached, :, j])), (j, out[:, :, j])
        assert np.max(np.abs(out[reached, 0, j] - sc.states[0, j] * np.cos(grid[reached]))) <= 1e-13
        assert (got[0][j]["outcome"] == RETIRED_BY_EVENT) == (sc.states[0, j] > 1.0)
    assert max(g["steps"] for g in got[0]) >= first_retirement + 3
    # propagate_grid_device(): the same samples in a caller-owned device buffer.
    import torch

    tb = hy.taylor_adaptive_batch(sc.system(hy), sc.states, 5, batch_semantics="independent", **sc.events(hy, 0))
    buf = torch.full((9, 2, 5), -1.0, dtype=torch.float64, device="cuda")
    tb.propagate_grid_device(grid, buf.data_ptr())
    assert np.array_equal(buf.cpu().numpy(), out, equal_nan=True) and tb.n_retired == 3
    assert [int(r[0]) for r in tb.propagate_res] == [g["outcome"] for g in got[0]]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: limits
# ---------------------------------------------------------------------------------------------------------------------
LIM_AMPS = np.array([0.5, 1.1, 0.9, 1.5, 3.0, 0.7, 0.8, 0.6])
LIM_TF = np.array([10.0, 10.0, 1.5, 10.0, 10.0, 2.0, 10.0, 1.0])


def _lim_scenario():
    sc = _osc_scenario(None, amps=LIM_AMPS)
    sc.tf = LIM_TF
    return sc


@pytest.mark.gpu
def test_max_steps_overrides_the_unfinished_systems_only():
    sc = _lim_scenario()
    ta, got, _ = _check(sc, range(8), [P_UNTIL(sc.tf, max_steps=5)], [O_UNTIL(sc.tf, max_steps=5)])
    assert [g["outcome"] for g in got[0]] == [int(OC.step_limit), -1, int(OC.time_limit), -1, -1, int(OC.time_limit),
                                              int(OC.step_limit), int(OC.time_limit)]
    assert [g["steps"] for g in got[0]][0] == 5


class _StopAfter:
    """Step callback which returns false at its k-th invocation."""

    def __init__(self, k):
        self.k, self.n = k, 0

    def __call__(self, ta):
        self.n += 1
        return self.n < self.k


@pytest.mark.gpu
def test_step_callback_stop_overrides_the_unfinished_systems_only():
    sc = _lim_scenario()

    def call(ta, idx):
        ta.propagate_until(sc.tf[idx] if ta.batch_size > 1 else float(sc.tf[idx[0]]), callback=_StopAfter(5))

    # (The oracle has no step callback: a callback which stops after the 5th sweep leaves the state max_steps = 5 leaves,
    # with cb_stop in place of step_limit.)
    def call_o(o, j):
        pr = o.propagate_until(float(sc.tf[j]), max_steps=5)
        return [((int(OC.cb_stop) if r[0] == int(OC.step_limit) else r[0]),) + tuple(r[1:]) for r in pr]

    ta, got, _ = _check(sc, range(8), [call], [call_o])
    assert [g["outcome"] for g in got[0]] == [int(OC.cb_stop), -1, int(OC.time_limit), -1, -1, int(OC.time_limit),
                                              int(OC.cb_stop), int(OC.time_limit)]


@pytest.mark.gpu
def test_a_non_finite_system_is_retired_alone():
    # x(0) = 1e14: x' = x^2 blows up at t = 1e-14, the oracle's 12th step is not finite (the Taylor coefficients, of
    # magnitude x^21, overflow); the healthy systems run on to t = 30 (14 and 21 steps) or to the event v = 0.2 (8 and 12).
    st = np.array([[1e14, -1.0, 0.0, -2.0, -0.5], [0.1, 1.0, 0.1, 1.0, 0.1]])
    sc = Blowup("blowup", st, np.full(5, 30.0))
    ta, got, ref = _check(sc, range(5), [P_UNTIL(sc.tf)], [O_UNTIL(sc.tf)])
    assert [g["outcome"] for g in got[0]] == [int(OC.err_nf_state), -1, int(OC.time_limit), -1, int(OC.time_limit)]
    # (The healthy systems were still running when the first one went non-finite.)
    assert got[0][0]["steps"] >= 5 and max(g["steps"] for g in got[0][1:]) >= got[0][0]["steps"] + 1 + 3
    assert abs(got[0][1]["time"][0] - np.log(5.0)) <= 1e-14 and got[0][2]["time"] == (30.0, 0.0)


@pytest.mark.gpu
def test_the_next_call_resumes_the_retired_systems():
    sc = _osc_scenario(None, amps=_amplitudes(5))
    tf2 = np.full(5, 20.0)
    ta, got, _ = _check(sc, range(5), [P_UNTIL(sc.tf), P_UNTIL(tf2)], [O_UNTIL(sc.tf), O_UNTIL(tf2)])
    for j, a in enumerate(sc.states[0]):
        if a > 1.0:
            # Retired at acos(1 / A), resumed, retired again one period later.
            assert got[0][j]["outcome"] == got[1][j]["outcome"] == RETIRED_BY_EVENT
            assert abs(got[1][j]["time"][0] - got[0][j]["time"][0] - 2.0 * np.pi) <= 1e-13
        else:
            assert got[1][j]["outcome"] == int(OC.time_limit) and got[1][j]["time"] == (20.0, 0.0)
