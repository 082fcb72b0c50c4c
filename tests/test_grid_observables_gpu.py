"""Grid observables on the MI355X. The yardstick is what exists without the feature: the same integrator
built twice, one runs ``propagate_grid(grid)`` and the other ``propagate_grid(grid, observables=obs)``; the expected rows
are ``hy.cfunc(obs, vars=state variables)`` of the full output, the parameters of the lane and the grid time of the row
where the whole state row was reached, NaN elsewhere. Every comparison is bit for bit (the NaN patterns as masks), and in
every test state, double-length times, propagate_res_arrays() and the Taylor coefficients of the two integrators are
identical."""
import os
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
OC = hy.taylor_outcome


def sys_vars(sys_):
    if isinstance(sys_, hy.var_ode_sys):
        return [p[0] for p in sys_.sys]
    return hy._to_sys(sys_).vars


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    """Bit for bit where neither is NaN, and the same NaN pattern."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def results(ta):
    oc, mn, mx, ns = ta.propagate_res_arrays()
    hi, lo = ta.dtime
    ret = dict(state=ta.state, t_hi=hi, t_lo=lo, outcome=np.asarray(oc), min_h=np.asarray(mn), max_h=np.asarray(mx),
               n_steps=np.asarray(ns))
    try:
        ret["tc"] = ta.tc
    except Exception as e:  # (an interrupted grid with coefficients on demand refuses them: the same refusal)
        ret["tc"] = np.array([hash(str(e))])
    return ret


def assert_identical(a, b, what=""):
    for k in a:
        assert same(a[k], b[k]), (what, k, a[k], b[k])


def expected(sys_, obs, out_full, pars, grid):
    """cfunc(obs)(out_full[g], pars, time=grid[g]) where the whole state row is non-NaN, NaN elsewhere: one evaluation
    over all the rows."""
    n_grid, dim, n = out_full.shape
    g2 = np.asarray(grid, dtype=float)
    if g2.ndim == 1:
        g2 = np.repeat(g2[:, None], n, axis=1)
    cf = hy.cfunc(obs, vars=sys_vars(sys_))
    np_ = cf.nparams
    inp = np.ascontiguousarray(out_full.transpose(1, 0, 2).reshape(dim, n_grid * n))
    vals = cf(inp, pars=np.tile(pars[:np_], (1, n_grid)) if np_ else None,
              time=g2.reshape(-1) if cf.is_time_dependent else None)
    vals = vals.reshape(len(obs), n_grid, n).transpose(1, 0, 2)
    reached = ~np.isnan(out_full).any(axis=1)
    return np.where(reached[:, None, :], vals, np.nan), reached


class _log_capture:
    def __enter__(self):
        self.msgs = []
        hy.set_log_callback(lambda lvl, m: self.msgs.append(m))
        hy.set_logger_level_debug()
        return self

    def __exit__(self, *exc):
        hy.set_logger_level("warn")
        hy.set_log_callback(None)

    def grid_lines(self):
        return [m for m in self.msgs if "propagate_grid() loop:" in m]


def run_pair(make, sys_, obs, grid, tas=None, make_cb=None, **kw):
    """(ta, tb, full output, observable output, reached mask, the debug line of the observable run)."""
    ta, tb = tas if tas is not None else (make(), make())
    kwa, kwb = dict(kw), dict(kw)
    if make_cb is not None:
        kwa["callback"], kwb["callback"] = make_cb(), make_cb()
    with _log_capture() as la:
        _, full = ta.propagate_grid(grid, **kwa)
    with _log_capture() as lb:
        _, out = tb.propagate_grid(grid, observables=obs, **kwb)
    assert out.shape == (full.shape[0], len(obs), full.shape[2])
    assert_identical(results(ta), results(tb))
    exp, reached = expected(sys_, obs, full, ta.pars, grid)
    ok = ~(np.isnan(out) | np.isnan(exp))
    diff = np.where(ok, bits(out).astype(np.int64) - bits(exp).astype(np.int64), 0)
    print("[grid observables] rows reached %d of %d, values which differ per observable %s (row 0: %s), largest distance "
          "in ulp %d" % (reached.sum(), reached.size, (diff != 0).sum(axis=(0, 2)).tolist(), (diff[0] != 0).sum(axis=1).tolist(),
                       np.abs(diff).max()))
    assert same(out, exp), (out, exp)
    # The choice of the loop and its launches are those of the call without observables.
    line_a, line_b = la.grid_lines()[0], lb.grid_lines()[0]
    assert line_b.startswith(line_a) and " observables over " in line_b[len(line_a):], (line_a, line_b)
    return ta, tb, full, out, reached, line_b


def lane_grid(n, t_end, n_pts, backward=False):
    """Per-lane grids: the same number of points, a spacing which differs from lane to lane by up to 3 %."""
    g = np.outer(np.linspace(0.0, t_end, n_pts), 1.0 + 0.03 * np.arange(n) / max(n - 1, 1))
    return -g if backward else g


def outer_ss_obs(sys_):
    vs = {repr(e): e for e in sys_vars(sys_)}
    d = [vs[a + "_1"] - vs[a + "_2"] for a in "xyz"]
    return [hy.model.nbody_energy(6, masses=M, Gconst=G), d[0] * d[0] + d[1] * d[1] + d[2] * d[2]]


# ---- 1. the headline path ----
def test_headline_multi_step_launches_forward_backward_and_staged(monkeypatch):
    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=41)
    obs = outer_ss_obs(sys_)
    grid = lane_grid(n, 30.0, 13)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    ta, tb, _, out, reached, line = run_pair(make, sys_, obs, grid)
    assert "v5" in tb.hip_source_mode
    assert reached.all()
    assert "multi-step launches" in line and "12 stepper launches for 12 grid intervals" in line, line
    assert "2 observables over 36 of 36 state rows, samples held in registers" in line, line
    # Backward over the same grid, back to the start, with the same two integrators.
    gb = grid[::-1].copy()
    _, _, _, outb, reached_b, _ = run_pair(None, sys_, obs, gb, tas=(ta, tb))
    assert reached_b.all()
    # The staging buffer gives the same bits.
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", "staged")
    tc = make()
    with _log_capture() as lc:
        _, out_s = tc.propagate_grid(grid, observables=obs)
        _, outb_s = tc.propagate_grid(gb, observables=obs)
    assert all("samples held in the staging buffer" in m and "multi-step launches" in m for m in lc.grid_lines())
    assert same(out_s, out) and same(outb_s, outb)
    assert_identical(results(tc), results(tb))


# ---- 2. batch sizes, scalar grids, a two-point grid ----
def pendulum():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.par[1] * hy.sin(x))]
    return sys_, x, v, [0.5 * v * v - hy.par[1] * hy.cos(x) + hy.par[0] * hy.sin(hy.time)]


def pendulum_inputs(n, seed=7):
    rng = np.random.RandomState(seed)
    st = np.stack([rng.uniform(0.1, 1.0, n), rng.uniform(-0.5, 0.5, n)])
    pars = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(5.0, 10.0, n)])
    return st, pars


@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_pendulum_batch_sizes_and_grid_kinds(n, ha):
    sys_, x, v, obs = pendulum()
    st, pars = pendulum_inputs(n)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, pars=pars, high_accuracy=ha)

    for grid in (lane_grid(n, 6.0, 7), np.linspace(0.0, 5.0, 5), np.array([0.0, 0.37]), lane_grid(n, 3.0, 4, backward=True)):
        *_, reached, line = run_pair(make, sys_, obs, grid)
        assert reached.all()
        assert "1 observables over 2 of 2 state rows" in line


def test_a_single_grid_point_is_row_zero():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    t0 = np.linspace(-1.0, 1.0, n)
    *_, out, reached, _ = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars, time=t0), sys_, obs, t0[None, :].copy())
    assert out.shape == (1, 1, n) and reached.all()


# ---- 3. single-step sweeps ----
def test_max_steps_between_two_grid_points_leaves_nan_in_every_column():
    """The tail rows are NaN in every column - also in the column of a comparison, whose cfunc of a NaN state is 0."""
    sys_, x, v, obs = pendulum()
    obs = obs + [hy.gt(x, -100.0), hy.gt(-100.0, x)]
    n = 5
    st, pars = pendulum_inputs(n)
    cf = hy.cfunc(obs, vars=[x, v])
    at_nan = cf(np.full((2, 1), np.nan), pars=pars[:, :1], time=np.zeros(1))
    assert at_nan[1, 0] == 0.0 and at_nan[2, 0] == 0.0
    grid = lane_grid(n, 2.0, 9)
    ta, tb, _, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), sys_, obs, grid, max_steps=9)
    assert "single-step sweeps" in line
    assert all(int(r[0]) == int(OC.step_limit) for r in tb.propagate_res)
    # (Some rows behind row 0 are reached in every lane, the last ones in none.)
    assert 1 < reached.all(axis=1).sum() < grid.shape[0] and not reached[-1].any()
    assert np.isnan(out[~reached.any(axis=1)]).all() and np.all(out[reached.all(axis=1)][:, 1] == 1.0)
    assert np.all(out[reached.all(axis=1)][:, 2] == 0.0)


class stop_after:
    def __init__(self, k):
        self.k, self.calls = k, 0

    def __call__(self, ta):
        self.calls += 1
        return self.calls < self.k


def test_python_step_callback_which_stops_the_loop():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, _, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), sys_, obs, grid,
                                            make_cb=lambda: stop_after(9))
    assert "single-step sweeps" in line and tb.last_callback_path == 1
    assert all(int(r[0]) == int(OC.cb_stop) for r in tb.propagate_res)
    assert 1 < reached.all(axis=1).sum() < grid.shape[0] and not reached[-1].any()


def test_counting_non_terminal_event():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 6.0, 7)
    cnts = []

    def make():
        cnts.append(hy.native_event_counter())
        return hy.taylor_adaptive_batch(sys_, st, n, pars=pars, nt_events=[hy.nt_event(v, cnts[-1])])

    ta, tb, _, out, reached, line = run_pair(make, sys_, obs, grid)
    assert "single-step sweeps" in line and reached.all()
    assert cnts[0].value == cnts[1].value > 0


# ---- 4. a lane which goes non-finite ----
def collision_state(n, d=2.25):
    """Outer Solar Systems; in lane 1 Jupiter falls radially onto the Sun from d AU: non-finite at t = 0.597 (the set-up of
    _collision_state in tests/test_grid_parity.py)."""
    st = configs.outer_ss_state(n, perturb=1e-6, seed=3).reshape(36, n).copy()
    st[6:9, 1] = st[0:3, 1] + np.array([d, 0.0, 0.0])
    st[9:12, 1] = st[3:6, 1]
    return st


@pytest.mark.parametrize("semantics", [None, "per_lane"])
def test_nonfinite_lane_rollback_and_per_lane(semantics):
    n = 67
    st = collision_state(n)
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    obs = outer_ss_obs(sys_)
    grid = np.linspace(0.0, 4.0, 9)
    ta, tb, full, out, reached, line = run_pair(
        lambda: hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, batch_semantics=semantics), sys_, obs, grid,
        max_delta_t=0.01)
    assert tb.propagate_res[1][0] == OC.err_nf_state
    assert ("rolled back to the start of the grid" in line) == (semantics is None), line
    # Row 0 (recomputed right after the rollback) and the row at t = 0.5 are there, the end of the grid is not.
    assert reached[0].all() and reached[1].all() and not reached[-1].any()
    assert not np.isnan(out[0]).any() and np.isnan(out[-1]).all()


# ---- 5. independent semantics ----
def osc():
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -x)], x, v


@pytest.mark.parametrize("n", [5, 65])
def test_independent_semantics_retired_systems(n):
    """A terminal event without a callback retires the systems whose amplitude reaches 1.2: their rows after the truncated
    step are NaN, and every system is bit for bit the system run alone with the same observables."""
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), x * v]
    st = np.stack([np.zeros(n), np.linspace(0.8, 1.6, n)])
    grid = lane_grid(n, 9.0, 10)

    def make(s=st, m=n):
        return hy.taylor_adaptive_batch(sys_, s, m, t_events=[hy.t_event(x - 1.2)], batch_semantics="independent")

    ta, tb, full, out, reached, line = run_pair(make, sys_, obs, grid)
    retired = np.array([int(r[0]) == -1 for r in tb.propagate_res])
    assert tb.n_retired == retired.sum() and 0 < retired.sum() < n
    assert reached[:, ~retired].all() and not reached[-1, retired].any() and reached[0].all()
    for i in range(n):
        t1 = make(st[:, i : i + 1].copy(), 1)
        _, o1 = t1.propagate_grid(grid[:, i : i + 1].copy(), observables=obs)
        assert same(o1[:, :, 0], out[:, :, i]), i


# ---- 6. other steppers ----
@pytest.mark.parametrize("emitter", [None, "table"])
def test_oscillator_unrolled_and_table_steppers(emitter):
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), hy.atan2(x, v), v]
    n = 5
    rng = np.random.RandomState(5)
    st = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])
    ta, tb, *_, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, emitter=emitter), sys_, obs,
                                         lane_grid(n, 7.0, 8))
    assert reached.all() and "3 observables over 2 of 2 state rows" in line
    if emitter:
        assert "table" in tb.hip_source_mode


def test_variational_pendulum_norm_of_the_tangent_vector():
    x, v = hy.make_vars("x", "v")
    vsys = hy.var_ode_sys([(x, v), (v, -9.8 * hy.sin(x))], [x], 1)
    svars = sys_vars(vsys)
    assert len(svars) == 4
    dx, dv = svars[2], svars[3]
    obs = [hy.sqrt(dx * dx + dv * dv)]
    n = 5
    rng = np.random.RandomState(11)
    st = np.stack([rng.uniform(0.1, 1.0, n), rng.uniform(-0.5, 0.5, n)])
    ta, tb, *_, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(vsys, st, n), vsys, obs, lane_grid(n, 5.0, 6))
    assert reached.all() and "1 observables over 2 of 4 state rows" in line
    assert np.all(out[0] == 1.0) and np.all(out > 0.0)


def test_literals_which_the_compiler_could_simplify_by_value():
    """The section holds its literals as opaque values in registers, the cfunc kernel sees them as literals: divisions by 3,
    by powers of two which are not inline constants, and functions of literal arguments give the same bits all the same."""
    sys_, x, v = osc()
    three, eight = hy.expression(3.0), hy.expression(8.0)
    obs = [x / 3.0, x / 8.0, v * 0.125 + x / 0.0625, hy.sin(three) * x + hy.exp(eight) * v, hy.pow(x * x + 1.0, three),
           hy.atan2(x, eight) + hy.sqrt(three) * v, 3.0 / (x * x + 8.0)]
    n = 65
    rng = np.random.RandomState(17)
    st = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])
    *_, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n), sys_, obs, lane_grid(n, 5.0, 6))
    assert reached.all() and "7 observables over 2 of 2 state rows" in line


# ---- 7. a caller-owned device buffer ----
def test_device_buffer_bits_and_extent():
    import torch

    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=48)
    obs = outer_ss_obs(sys_)
    sentinel = -1234.5

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    for grid in (lane_grid(n, 10.0, 6), np.linspace(0.0, 8.0, 5)):
        ta, tb = make(), make()
        _, out = ta.propagate_grid(grid, observables=obs)
        count = grid.shape[0] * len(obs) * n
        buf = torch.full((count + 4096,), sentinel, dtype=torch.float64, device="cuda")
        tb.propagate_grid_device(grid, buf.data_ptr(), observables=obs)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert same(host[:count].reshape(out.shape), out)
        assert not np.any(host[:count] == sentinel) and np.all(host[count:] == sentinel)
        assert_identical(results(ta), results(tb))


# ---- 8. run to run, batch size and position ----
def test_run_to_run_and_batch_independence():
    sys_, x, v, obs = pendulum()
    n = 65
    st, pars = pendulum_inputs(n, seed=13)
    grid = lane_grid(n, 6.0, 7)

    def run(idx):
        idx = np.asarray(idx)
        ta = hy.taylor_adaptive_batch(sys_, st[:, idx].copy(), len(idx), pars=pars[:, idx].copy(), high_accuracy=True)
        return ta.propagate_grid(grid[:, idx].copy(), observables=obs)[1]

    a, b = run(np.arange(n)), run(np.arange(n))
    assert same(a, b) and not np.isnan(a).any()
    for idx in ([64], [7], [3, 64, 7], list(reversed(range(n)))):
        o = run(idx)
        assert same(o, a[:, :, idx]), idx


# ---- 9. the C++ program ----
def test_cpp_grid_observables_on_gpu():
    from test_grid_observables import build_cpp

    out = subprocess.run([build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
