"""step_action on the MI355X. The yardsticks are the two things which exist without the feature: the same
thing written as a Python host callback - values from hy.cfunc on host arrays, the mask ``ta.last_h != 0``, written
through ``ta.state``, ``not any(cond[mask])`` returned - and, for the independent semantics, the same system run alone
in a batch of one. Every comparison is bit for bit."""
import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

pytestmark = pytest.mark.gpu

CB_STOP = int(hy.taylor_outcome.cb_stop)
TIME_LIMIT = int(hy.taylor_outcome.time_limit)
TWOPI = float.fromhex("0x1.921fb54442d18p+2")


def sys_vars(sys_):
    if isinstance(sys_, hy.var_ode_sys):
        return [p[0] for p in sys_.sys]
    return hy._to_sys(sys_).vars


class host_action:
    """The action restated as a host callback: what a user had to write before, and the reference of the comparisons."""

    def __init__(self, sys_, assignments, stop_when=None):
        svars = sys_vars(sys_)
        names = [repr(s) for s in svars]
        pairs = list(assignments.items()) if isinstance(assignments, dict) else list(assignments or ())
        self.rows = [names.index(repr(lhs)) for lhs, _ in pairs]
        self.cond = stop_when is not None
        fn = [rhs for _, rhs in pairs]
        self.cf = hy.cfunc(fn + ([stop_when] if self.cond else []), vars=svars)
        self.calls = 0

    def values(self, ta, st):
        np_ = self.cf.nparams
        return self.cf(st, pars=ta.pars[:np_] if np_ else None, time=ta.time if self.cf.is_time_dependent else None)

    def __call__(self, ta):
        self.calls += 1
        st = ta.state
        mask = ta.last_h != 0
        out = self.values(ta, st)
        for k, row in enumerate(self.rows):
            st[row, mask] = out[k, mask]
        ta.state = st
        if self.cond:
            return not np.any(out[-1][mask] != 0)
        return True


def results(ta):
    oc, mn, mx, ns = ta.propagate_res_arrays()
    hi, lo = ta.dtime
    return dict(state=ta.state, t_hi=hi, t_lo=lo, outcome=np.asarray(oc), min_h=np.asarray(mn), max_h=np.asarray(mx),
                n_steps=np.asarray(ns))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_identical(a, b, what=""):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, a[k], b[k])


def run_pair(make, sys_, assignments, stop_when, tf, call="propagate_until", **kw):
    ta, tb = make(), make()
    act = hy.step_action(assignments, stop_when=stop_when)
    host = host_action(sys_, assignments, stop_when)
    ra = getattr(ta, call)(tf, callback=act, **kw)
    rb = getattr(tb, call)(tf, callback=host, **kw)
    assert ta.last_callback_path == 4 and tb.last_callback_path == 1, (ta.last_callback_path, tb.last_callback_path)
    assert host.calls >= 3
    assert_identical(results(ta), results(tb))
    return ta, tb, ra, rb, host


def spread_tf(n, lo, hi):
    """Per-system final times: the first systems are done several sweeps before the last ones."""
    return np.linspace(lo, hi, n) if n > 1 else np.array([hi])


# ---- 1. bit for bit against the host callback ----
def osc():
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -x)], x, v


def osc_state(n, seed=5):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])


@pytest.mark.parametrize("which", ["damp", "swap"])
@pytest.mark.parametrize("n,emitter", [(1, None), (3, None), (64, None), (65, None), (1, "table"), (5, "table")])
def test_oscillator_matches_the_host_callback(n, emitter, which):
    sys_, x, v = osc()
    st0 = osc_state(n)
    asg = {v: (1 - 1e-3) * v} if which == "damp" else [(x, v), (v, x)]
    ta, _, _, _, host = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st0, n, emitter=emitter), sys_, asg, None,
                                 spread_tf(n, 2.0, 12.0))
    if emitter:
        assert "table" in ta.hip_source_mode
    # (The mask was exercised: the first system was done while the last one was still stepping.)
    assert n == 1 or results(ta)["n_steps"][0] + 2 < results(ta)["n_steps"][-1]


def test_pendulum_with_parameters_and_time():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.par[1] * hy.sin(x))]
    n = 7
    rng = np.random.RandomState(2)
    st0 = np.stack([rng.uniform(0.0, 1.0, n), rng.uniform(2.0, 3.0, n)])
    pars = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(5.0, 10.0, n)])
    t0 = rng.uniform(-1.0, 1.0, n)
    run_pair(lambda: hy.taylor_adaptive_batch(sys_, st0, n, pars=pars, time=t0), sys_, {v: v + hy.par[0] * hy.cos(hy.time)},
             None, t0 + spread_tf(n, 1.0, 4.0))


def test_outer_solar_system_two_wavefronts():
    """One lane per pair of bodies: 5 systems span two wavefronts of the stepper."""
    sys_ = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
    vs = {repr(e): e for e in sys_vars(sys_)}
    n = 5
    st0 = configs.outer_ss_state(n, perturb=1e-3, seed=3)
    asg = {vs[k]: (1.0 + 1e-12) * vs[k] for k in ("vx_1", "vy_1", "vz_1")}
    ta, *_ = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st0, n, high_accuracy=True), sys_, asg, None, spread_tf(n, 2.0, 8.0))
    assert "cluster" in ta.hip_source_mode


def test_variational_tangent_renormalised():
    sys_, x, v = osc()
    vsys = hy.var_ode_sys(sys_, [x], 1)
    svars = sys_vars(vsys)
    assert len(svars) == 4
    dx, dv = svars[2], svars[3]
    nrm = hy.sqrt(dx * dx + dv * dv)
    n = 5
    st0 = osc_state(n)
    ta, *_ = run_pair(lambda: hy.taylor_adaptive_batch(vsys, st0, n), vsys, [(dx, dx / nrm), (dv, dv / nrm)], None,
                      spread_tf(n, 2.0, 9.0))
    st = ta.state
    assert np.all(np.abs(st[2] ** 2 + st[3] ** 2 - 1.0) < 1e-2)


# ---- 2. direct call ----
def test_direct_call_writes_the_bits_of_cfunc():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.par[1] * hy.sin(x))]
    n = 65
    rng = np.random.RandomState(9)
    st0 = np.stack([rng.uniform(0.0, 1.0, n), rng.uniform(2.0, 3.0, n)])
    pars = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(5.0, 10.0, n)])
    ta = hy.taylor_adaptive_batch(sys_, st0, n, pars=pars, time=rng.uniform(-1.0, 1.0, n))
    asg = {v: v + hy.par[0] * hy.cos(hy.time)}
    act, host = hy.step_action(asg), host_action(sys_, asg)
    # A fresh integrator: no system has taken a step, nothing happens.
    assert act(ta) is True
    assert np.array_equal(bits(ta.state), bits(st0))
    ta.step()
    pre = ta.state
    want = host.values(ta, pre)
    tc, lh, tm = ta.tc, ta.last_h, ta.dtime
    assert act(ta) is True
    post = ta.state
    assert np.array_equal(bits(post[1]), bits(want[0])) and not np.array_equal(bits(post[1]), bits(pre[1]))
    assert np.array_equal(bits(post[0]), bits(pre[0]))
    assert np.array_equal(bits(ta.tc), bits(tc)) and np.array_equal(bits(ta.last_h), bits(lh))
    assert np.array_equal(bits(ta.dtime[0]), bits(tm[0])) and np.array_equal(bits(ta.dtime[1]), bits(tm[1]))
    # With the host mirror the newer copy (a state set by value): uploaded first, the same bits.
    ta.state = pre
    assert act(ta) is True
    assert np.array_equal(bits(ta.state), bits(post))
    # The stop condition of a direct call: False when it holds for a system which took a step.
    assert hy.step_action(stop_when=hy.gt(v, 0.0))(ta) is False
    assert hy.step_action(stop_when=hy.gt(v, 1e3))(ta) is True
    assert np.array_equal(bits(ta.state), bits(post))


# ---- 3. stop_when, default semantics ----
@pytest.mark.parametrize("n", [3, 65])
def test_stop_when_ends_the_loop_like_a_host_callback(n):
    sys_, x, v = osc()
    # x = -a sin t under a slight damping: the largest amplitudes reach x > 1.2 a little after t = pi, a few sweeps in.
    st0 = np.stack([np.zeros(n), -np.linspace(0.5, 1.5, n)])
    ta, tb, _, _, host = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st0, n), sys_, {v: (1 - 1e-3) * v}, hy.gt(x, 1.2),
                                  50.0)
    r = results(ta)
    # The loop ended early, at the sweep at which the host callback returned false: every system reports cb_stop.
    assert np.all(r["outcome"] == CB_STOP) and np.all(r["t_hi"] < 50.0)
    assert np.all(r["n_steps"] == host.calls)
    assert ta.n_stopped_by_action == 0


# ---- 4. stop_when, independent semantics ----
def solo_results(sys_, st0, i, act, tf, grid=None):
    t1 = hy.taylor_adaptive_batch(sys_, st0[:, i:i + 1], 1)
    if grid is not None:
        return t1, t1.propagate_grid(grid[:, i:i + 1], callback=act)[1]
    t1.propagate_until(tf[i:i + 1], callback=act)
    return t1, None


@pytest.mark.parametrize("n", [5, 65])
def test_stop_when_retires_one_system_under_independent_semantics(n):
    sys_, x, v = osc()
    # x = -a sin t under a slight damping: the systems with a well above 1.1 reach x > 1.1 a little after t = pi - a few
    # sweeps in, and before their final times -, the others never do.
    st0 = np.stack([np.zeros(n), -np.linspace(0.6, 1.6, n)])
    act = hy.step_action({v: (1 - 1e-3) * v}, stop_when=hy.gt(x, 1.1))
    tf = spread_tf(n, 4.0, 9.0)
    ta = hy.taylor_adaptive_batch(sys_, st0, n, batch_semantics="independent")
    for rep in range(2):
        # (A second call starts every system again.)
        ta.state, ta.time = st0, np.zeros(n)
        ta.propagate_until(tf, callback=act)
        assert ta.last_callback_path == 4
        r = results(ta)
        stopped = int(np.sum(r["outcome"] == CB_STOP))
        assert 0 < stopped < n, r["outcome"]
        assert ta.n_stopped_by_action == stopped and ta.n_retired == 0
        assert set(r["outcome"].tolist()) == {CB_STOP, TIME_LIMIT}
        assert np.all(r["t_hi"][r["outcome"] == TIME_LIMIT] == tf[r["outcome"] == TIME_LIMIT])
        if rep == 0:
            first = r
        else:
            assert_identical(r, first, "second call")
    for i in range(n):
        t1, _ = solo_results(sys_, st0, i, act, tf)
        r1 = results(t1)
        for k in r:
            assert np.array_equal(bits(r[k][..., i:i + 1]), bits(r1[k])), (i, k, r[k][..., i], r1[k])
    # propagate_grid(): the rows of a stopped system stay NaN from its stop on, like alone.
    grid = np.linspace(0.0, 1.0, 9)[:, None] * tf[None, :]
    tg = hy.taylor_adaptive_batch(sys_, st0, n, batch_semantics="independent")
    out = tg.propagate_grid(grid, callback=act)[1]
    assert tg.last_callback_path == 4
    rg = results(tg)
    assert 0 < tg.n_stopped_by_action == int(np.sum(rg["outcome"] == CB_STOP)) < n
    for i in range(n):
        t1, o1 = solo_results(sys_, st0, i, act, tf, grid)
        assert np.array_equal(np.isnan(out[:, :, i]), np.isnan(o1[:, :, 0])), (i, out[:, :, i], o1[:, :, 0])
        ok = ~np.isnan(o1[:, :, 0])
        assert np.array_equal(bits(out[:, :, i][ok]), bits(o1[:, :, 0][ok]))
        r1 = results(t1)
        for k in rg:
            assert np.array_equal(bits(rg[k][..., i:i + 1]), bits(r1[k])), (i, k, rg[k][..., i], r1[k])
    assert np.isnan(out[-1, 0, n - 1]) and not np.isnan(out[-1, 0, 0])


# ---- 5. sets ----
class host_reducer:
    def __init__(self, idx):
        self.idx = list(idx)

    def __call__(self, ta):
        st = ta.state
        st[self.idx] = st[self.idx] - TWOPI * np.floor(st[self.idx] / TWOPI)
        ta.state = st
        return True


class recorder:
    def __init__(self):
        self.states = []

    def __call__(self, ta):
        self.states.append(ta.state)
        return True


def rotating():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.sin(x))]
    st0 = np.stack([np.linspace(0.0, 1.0, 5), np.linspace(9.0, 11.0, 5)])
    return sys_, x, v, st0


def test_set_with_the_angle_reducer_is_library_side():
    sys_, x, v, st0 = rotating()
    asg = {v: (1 - 1e-3) * v}
    ta, tb = (hy.taylor_adaptive_batch(sys_, st0, 5) for _ in range(2))
    tf = spread_tf(5, 1.0, 3.0)
    ta.propagate_until(tf, callback=[hy.step_action(asg), hy.callback.angle_reducer([x])])
    tb.propagate_until(tf, callback=[host_action(sys_, asg), host_reducer([0])])
    assert ta.last_callback_path == 4 and tb.last_callback_path == 1
    assert_identical(results(ta), results(tb))
    assert np.all(ta.state[0] < TWOPI) and np.all(ta.state[0] >= 0)
    # A set of angle reducers alone keeps its own paths.
    tc = hy.taylor_adaptive_batch(sys_, st0, 5)
    tc.propagate_until(tf, callback=[hy.callback.angle_reducer([x])])
    assert tc.last_callback_path in (2, 3)


def test_set_with_a_python_callback_keeps_the_order():
    sys_, x, v, st0 = rotating()
    asg = {v: 0.5 * v}
    tf = spread_tf(5, 1.0, 3.0)
    recs = {}
    for name, make in (("act_first", lambda r: [hy.step_action(asg), r]), ("host_first", lambda r: [host_action(sys_, asg), r]),
                       ("act_last", lambda r: [r, hy.step_action(asg)]), ("host_last", lambda r: [r, host_action(sys_, asg)])):
        t = hy.taylor_adaptive_batch(sys_, st0, 5)
        r = recorder()
        t.propagate_until(tf, callback=make(r))
        assert t.last_callback_path == 1
        recs[name] = (np.array(r.states), results(t))
    for a, b in (("act_first", "host_first"), ("act_last", "host_last")):
        assert np.array_equal(bits(recs[a][0]), bits(recs[b][0]))
        assert_identical(recs[a][1], recs[b][1])
    # The Python callback sees the changed state behind the action, the unchanged one in front of it: v was halved.
    assert_identical(recs["act_first"][1], recs["act_last"][1])
    assert np.array_equal(bits(recs["act_first"][0][0, 1]), bits(0.5 * recs["act_last"][0][0, 1]))
    assert np.array_equal(bits(recs["act_first"][0][0, 0]), bits(recs["act_last"][0][0, 0]))


# ---- 6. with events ----
def test_next_to_a_counting_event():
    sys_, x, v = osc()
    n = 5
    st0 = osc_state(n)
    asg = {v: (1 - 1e-3) * v}
    ca, cb = hy.native_event_counter(), hy.native_event_counter()
    ta = hy.taylor_adaptive_batch(sys_, st0, n, nt_events=[hy.nt_event(v, ca)])
    tb = hy.taylor_adaptive_batch(sys_, st0, n, nt_events=[hy.nt_event(v, cb)])
    tf = spread_tf(n, 4.0, 12.0)
    ta.propagate_until(tf, callback=hy.step_action(asg))
    tb.propagate_until(tf, callback=host_action(sys_, asg))
    assert ta.last_callback_path == 4 and tb.last_callback_path == 1
    assert ca.value == cb.value and ca.value >= n
    assert_identical(results(ta), results(tb))


# ---- 7. with continuous output ----
def test_with_continuous_output():
    sys_, x, v = osc()
    n = 5
    st0 = osc_state(n)
    asg = {v: (1 - 1e-3) * v}
    _, _, ra, rb, _ = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st0, n), sys_, asg, None, spread_tf(n, 3.0, 9.0),
                               c_output=True)
    ca, cb = ra[0], rb[0]
    assert ca is not None and cb is not None and ca.n_steps == cb.n_steps
    for tm in (0.5, 1.7, 2.9):
        assert np.array_equal(bits(np.array(ca(tm))), bits(np.array(cb(tm))))


# ---- 8. batch-size independence ----
@pytest.mark.parametrize("amp,stops", [(0.8, False), (1.6, True)])
def test_results_do_not_depend_on_batch_size_or_position(amp, stops):
    sys_, x, v = osc()
    act = hy.step_action({v: (1 - 1e-3) * v}, stop_when=hy.gt(x, 1.1))
    mine = np.array([[0.0], [-amp]])
    ref = None
    for n in (1, 2, 3, 63, 64, 65):
        for pos in sorted({0, n - 1}):
            rng = np.random.RandomState(100 + n)
            st0 = np.stack([np.zeros(n), -rng.uniform(0.6, 1.6, n)])
            tf = rng.uniform(3.0, 9.0, n)
            st0[:, pos:pos + 1] = mine
            tf[pos] = 7.0
            ta = hy.taylor_adaptive_batch(sys_, st0, n, batch_semantics="independent")
            ta.propagate_until(tf, callback=act)
            r = {k: a[..., pos] for k, a in results(ta).items()}
            assert (r["outcome"] == CB_STOP) == stops
            if ref is None:
                ref = r
            else:
                assert_identical(r, ref, (n, pos))
