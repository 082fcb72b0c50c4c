"""Event-log observables on the GPU. Integrator S logs the state columns, integrator O the observables, from
the same initial data; every comparison is exact:
- columns 0-7 of O's rows are those of S, in order, and the integrators stay equal step by step;
- every observable column equals cfunc(observables, vars = state variables) of S's state columns, the parameters of the
  row's system and time = column 4;
- the mixed path (a recorder next to a Python callback: the host loop) against the device path, whole rows;
- the staging buffer against the registers, whole logs, each mode in a process of its own;
- the rows of a system do not depend on the batch; the life cycle of the list.
The configurations are those of tests/test_event_recorder.py - pendulum (unrolled stepper), outer Solar System on the v5
stepper (events inside the stepper, compact coefficients) and on v2 - and two with runtime parameters, so that the
parameters of the row's system matter: a pendulum with one gravity per system, the outer Solar System with par[] masses."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ["pendulum", "outer_ss_v5", "outer_ss_v2", "pendulum_par", "outer_ss_par"]
N_SYS, N_STEPS = 1024, 12


def _pendulum(with_par=False):
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -(hy.par[0] if with_par else 9.8) * hy.sin(x))], x, v


def _state_vars(sys_):
    return sys_.vars if hasattr(sys_, "vars") else [lhs for lhs, _ in sys_]


@functools.lru_cache(maxsize=None)
def _outer_ss_spread():
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    rng = np.random.RandomState(5)
    sysd = hy.model.nbody(6, masses=M, Gconst=G)
    spread = hy.taylor_adaptive_batch(sysd, configs.outer_ss_state(N_SYS, perturb=1e-6, seed=31), N_SYS, high_accuracy=True)
    # (The ensemble of tests/test_event_recorder.py spreads its systems over 30 years and logs some 200 rows per step. Here
    # half of them sit within 0.75 years of each other - about one step: they cross the plane y_1 = 0, twice per period of
    # 11.9 years, inside one or two steps, so that a single step logs more rows than a workgroup of the row kernel holds.)
    tf = np.concatenate([rng.uniform(0.0, 30.0, N_SYS // 2), rng.uniform(0.0, 0.75, N_SYS - N_SYS // 2)])
    spread.propagate_until(rng.permutation(tf))
    return np.array(spread.state)


def _setup(config):
    """(system, state, parameters or None, non-terminal event equations, terminal event equation, observables, keyword
    arguments): the ensembles of tests/test_event_recorder.py."""
    if config.startswith("pendulum"):
        with_par = config == "pendulum_par"
        sys_, x, v = _pendulum(with_par)
        rng = np.random.RandomState(11)
        st = np.stack([rng.uniform(-1.4, 1.4, N_SYS), rng.uniform(-2.0, 2.0, N_SYS)])
        pars = rng.uniform(9.0, 10.5, (1, N_SYS)) if with_par else None
        g = hy.par[0] if with_par else 9.8
        # (x alone, v alone, both, the time, a plain copy of a row and a number.)
        obs = [hy.sin(x), v * v, 0.5 * v * v - g * hy.cos(x), hy.time * v + x, x, hy.time]
        return sys_, st, pars, [v, x - 0.02], x + 0.03, obs, {}
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    with_par = config == "outer_ss_par"
    masses = [hy.par[i] for i in range(6)] if with_par else M
    sysd = hy.model.nbody(6, masses=masses, Gconst=G)
    pars = None
    if with_par:
        rng = np.random.RandomState(17)
        pars = np.array(M)[:, None] * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, (6, N_SYS)))
    var = {repr(e): e for e in _state_vars(sysd)}
    p = lambda i: [var["%s_%d" % (c, i)] for c in "xyz"]  # noqa: E731
    w = lambda i: [var["v%s_%d" % (c, i)] for c in "xyz"]  # noqa: E731
    # On the compact layout a position is a derived row (sampled from its velocity's coefficients), a velocity its parent:
    # positions only, velocities only, both of one body, all 36 rows with the masses, the time next to a row.
    obs = [hy.sum([(a - b) * (a - b) for a, b in zip(p(1), p(4))]),
           hy.sum([a * a for a in w(2)]),
           hy.sum([a * b for a, b in zip(p(3), w(3))]),
           hy.model.nbody_energy(6, masses=masses, Gconst=G),
           hy.time + var["y_1"]]
    kw = {"cluster_kernel": "v2"} if config == "outer_ss_v2" else {}
    return sysd, _outer_ss_spread(), pars, [var["y_1"], var["y_2"]], var["y_3"], obs, kw


def _make(config, ha, n=None, host_cb=None, **more):
    """An integrator of the configuration over its first n systems with recorders on every event; host_cb: the index of the
    non-terminal event which gets a do-nothing Python callback instead (the host loop)."""
    sys_, st, pars, nt_eqs, t_eq, obs, kw = _setup(config)
    n = st.shape[1] if n is None else n
    cbs = [(lambda *args: None) if host_cb == k else hy.native_event_recorder() for k in range(2)]
    if pars is not None:
        kw = dict(kw, pars=pars[:, :n])
    return hy.taylor_adaptive_batch(sys_, st[:, :n], n, high_accuracy=ha, nt_events=[hy.nt_event(nt_eqs[0], cbs[0]), hy.nt_event(nt_eqs[1], cbs[1])],
                                    t_events=[hy.t_event(t_eq, hy.native_event_recorder(), cooldown=0.05)], **kw, **more)


def _expected(config, s_rows):
    """cfunc(observables, vars = state variables) of the state columns of S's rows, the parameters of the row's system and
    time = column 4: (rows, n_obs)."""
    sys_, _, pars, _, _, obs, _ = _setup(config)
    cf = hy.cfunc(obs, _state_vars(sys_))
    lanes = s_rows[:, 0].astype(int)
    return cf(np.ascontiguousarray(s_rows[:, 8:].T), pars=None if pars is None else np.ascontiguousarray(pars[:, lanes]),
              time=np.ascontiguousarray(s_rows[:, 4])).T


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def _run(config, ha):
    """S: the state columns. O: the observables. C / C2: O with a Python callback on the second / first non-terminal event."""
    obs = _setup(config)[5]
    s, o, c, c2 = _make(config, ha), _make(config, ha), _make(config, ha, host_cb=1), _make(config, ha, host_cb=0)
    for ta in (o, c, c2):
        ta.event_log_observables = obs
    assert o.event_stats["events_on_device"] and not c.event_stats["events_on_device"]
    same, per_step = [], []
    for _ in range(N_STEPS):
        n0 = o.event_log_size
        for ta in (s, o, c, c2):
            ta.step()
        same.append(all(np.array_equal(s.state, ta.state) and np.array_equal(s.time, ta.time) and s.step_res == ta.step_res
                        and s.te_cooldowns == ta.te_cooldowns for ta in (o, c, c2)))
        per_step.append(o.event_log_size - n0)
    return {"mode": o.hip_source_mode, "same": same, "per_step": per_step, "s": s.event_log.rows, "o": o.event_log,
            "c": c.event_log.rows, "c2": c2.event_log.rows, "n_obs": len(obs), "dim": s.dim}


def _check_mode(config, mode):
    if config.startswith("pendulum"):
        assert "unrolled" in mode, mode
    elif config == "outer_ss_v5":
        assert "v5" in mode and "inside the stepper" in mode, mode
    elif config == "outer_ss_v2":
        assert "v2" in mode and "inside the stepper" not in mode, mode


@pytest.mark.gpu
@pytest.mark.parametrize("ha", [True, False])
@pytest.mark.parametrize("config", CONFIGS)
def test_observables_equal_cfunc_of_the_state_columns(config, ha):
    """Test 1."""
    r = _run(config, ha)
    _check_mode(config, r["mode"])
    assert all(r["same"]), r["same"]
    sr, ol = r["s"], r["o"]
    assert sr.shape == (len(ol), 8 + r["dim"]) and ol.rows.shape == (len(ol), 8 + r["n_obs"])
    assert ol.state is None and ol.observables.shape == (len(ol), r["n_obs"])
    assert _same_bits(sr[:, :8], ol.rows[:, :8])
    # (What the inputs must produce: both classes of row, and a step whose rows cross a workgroup of the row kernel.)
    n_term = int(np.sum(ol.terminal))
    assert n_term >= 1 and len(ol) - n_term >= 1 and max(r["per_step"]) > 256, (n_term, len(ol), r["per_step"])
    exp = _expected(config, sr)
    bad = np.flatnonzero(np.any(exp.view(np.uint64) != np.ascontiguousarray(ol.observables).view(np.uint64), axis=1))
    print("[event observables vs cfunc] %s ha=%s (%s): %d rows, %d terminal, rows per step %s, %d rows differ"
          % (config, ha, r["mode"].split(" [")[0], len(ol), n_term, r["per_step"], bad.size))
    assert bad.size == 0, (bad[:10], ol.rows[bad[:3]], exp[bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("ha", [True, False])
@pytest.mark.parametrize("config", CONFIGS)
def test_mixed_path_equals_device_path(config, ha):
    """Test 2. The rows of the events the recorders share, whole rows: the host loop collects the headers, hy_obs_rows fills
    the observables behind them."""
    r = _run(config, ha)
    al = r["o"].rows
    for other, idx in ((r["c"], 1), (r["c2"], 0)):
        keep = ~((al[:, 1] == 1) & (al[:, 2] == idx))
        assert 0 < np.sum(keep) < al.shape[0] and other.shape[1] == 8 + r["n_obs"]
        assert _same_bits(al[keep], other)


# ---- test 3: the staging buffer against the registers, each in a process of its own ----
def _child(config, mode, out):
    assert os.environ["HEYOKA_AMD_EVENT_OBS"] == mode
    ta = _make(config, True)
    ta.event_log_observables = _setup(config)[5]
    assert ("a.stage" in ta.event_log_source(2).split("hy_obs_rows(const")[1]) == (mode == "staged")
    for _ in range(6):
        ta.step()
    np.save(out, ta.event_log.rows)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["pendulum", "outer_ss_v5"])
def test_staged_equals_registers(config, tmp_path):
    logs = []
    for mode in ("registers", "staged"):
        out = str(tmp_path / (mode + ".npy"))
        env = dict(os.environ, HEYOKA_AMD_EVENT_OBS=mode, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), config, mode, out], env=env, capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        logs.append(np.load(out))
    assert logs[0].shape[0] > 256 and _same_bits(logs[0], logs[1])
    # (... and the registers of the child are those of this process: the default below 64 rows read.)
    r = _run(config, True)
    assert _same_bits(r["o"].rows[:logs[0].shape[0]], logs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257])
def test_rows_of_a_system_do_not_depend_on_the_batch(n):
    """Test 4."""
    big = _run("pendulum_par", False)["o"].rows
    ta = _make("pendulum_par", False, n=n)
    ta.event_log_observables = _setup("pendulum_par")[5]
    for _ in range(N_STEPS):
        ta.step()
    ref = big[big[:, 0] < n]
    assert np.sum(ref[:, 0] == 0) > 0 and _same_bits(ta.event_log.rows, ref)


@pytest.mark.gpu
def test_life_cycle(monkeypatch):
    """Test 5."""
    config, n = "pendulum_par", 512
    obs = _setup(config)[5]
    s, o = _make(config, False, n=n), _make(config, False, n=n)
    o.event_log_observables = obs
    s.propagate_until(0.6)
    o.propagate_until(0.6)
    n1 = o.event_log_size
    assert n1 == s.event_log_size > 100 and _same_bits(o.event_log.observables, _expected(config, s.event_log.rows))
    # The setter is refused on a non-empty log - setting and clearing alike -, and accepted once the log is cleared.
    for value in (None, obs[:2]):
        with pytest.raises(ValueError, match="only while the log is empty"):
            o.event_log_observables = value
    assert o.event_log_row_size == 8 + len(obs) and o.event_log_size == n1
    # (The states switch has no effect while observables are set: it moves freely, rows or not.)
    o.event_log_states = False
    o.event_log_states = True
    assert o.event_log_row_size == 8 + len(obs) and o.event_log_size == n1
    o.clear_event_log()
    o.event_log_observables = obs[:2]
    assert o.event_log_row_size == 10 and o.event_log_size == 0
    # A copy records on its own, with the list of the original.
    c = o.copy()
    for ta in (s, c):
        ta.clear_event_log()
        ta.propagate_until(0.9)
    assert c.event_log_size == s.event_log_size > 0 and o.event_log_size == 0
    assert _same_bits(c.event_log.observables, _expected(config, s.event_log.rows)[:, :2])
    # The log grows, with the staging buffer, past its reserve: staged mode, a reserve of one step's rows.
    monkeypatch.setenv("HEYOKA_AMD_EVENT_OBS", "staged")
    g, gs = _make(config, False, n=n), _make(config, False, n=n)
    g.event_log_observables = obs
    assert "a.stage" in g.event_log_source(2).split("hy_obs_rows(const")[1]
    monkeypatch.delenv("HEYOKA_AMD_EVENT_OBS")
    caps = []
    for _ in range(N_STEPS):
        g.step()
        gs.step()
        caps.append(g.event_log_capacity)
    assert g.event_log_size > caps[0] >= 1024 and caps[-1] > caps[0], (caps, g.event_log_size)
    assert _same_bits(g.event_log.rows[:, :8], gs.event_log.rows[:, :8])
    assert _same_bits(g.event_log.observables, _expected(config, gs.event_log.rows))


@pytest.mark.gpu
def test_independent_semantics_logs_the_last_events_of_retired_systems():
    """Test 5, last item. A stopping terminal event retires a system (batch_semantics="independent"); the rows of the
    recorders - the terminal one included - of the step in which it retires hold the observables like any other."""
    sys_, x, v = _pendulum(True)
    n = 512
    rng = np.random.RandomState(23)
    st = np.stack([rng.uniform(-0.3, 0.1, n), rng.uniform(1.0, 3.0, n)])
    pars = rng.uniform(9.0, 10.5, (1, n))
    obs = [0.5 * v * v - hy.par[0] * hy.cos(x), hy.time, x]

    def mk():
        return hy.taylor_adaptive_batch(sys_, st, n, pars=pars, batch_semantics="independent",
                                        nt_events=[hy.nt_event(v, hy.native_event_recorder())],
                                        t_events=[hy.t_event(x, hy.native_event_recorder(), cooldown=0.05),
                                                  hy.t_event(x - 0.5, direction=hy.event_direction.positive)])

    s, o = mk(), mk()
    o.event_log_observables = obs
    assert o.event_stats["events_on_device"]
    s.propagate_until(1.5)
    o.propagate_until(1.5)
    assert np.array_equal(s.state, o.state) and np.array_equal(s.time, o.time) and s.propagate_res == o.propagate_res
    sl, ol = s.event_log, o.event_log
    assert _same_bits(sl.rows[:, :8], ol.rows[:, :8])
    cf = hy.cfunc(obs, [x, v])
    exp = cf(np.ascontiguousarray(sl.state.T), pars=np.ascontiguousarray(pars[:, sl.system]), time=np.ascontiguousarray(sl.time)).T
    assert _same_bits(ol.observables, exp)
    retired = np.flatnonzero(np.array(o.time) < 1.5)
    assert o.n_retired == retired.size > 10 and retired.size < n
    # The retired systems crossed x = 0 (the terminal recorder) on their way to x = 0.5: their last rows are there.
    with_t_row = np.unique(ol.system[ol.terminal])
    assert np.intersect1d(retired, with_t_row).size > 10
    print("[event observables, independent] %d rows, %d systems retired, %d of them with a terminal row" % (len(ol), retired.size, np.intersect1d(retired, with_t_row).size))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3])
