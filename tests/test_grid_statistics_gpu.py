"""Grid statistics on the MI355X. The yardstick is what exists without the feature: the same integrator built
twice, one runs ``propagate_grid(grid, observables=obs)`` and the other adds ``statistics=``; the expected values are the
fold of the table of the design - an explicit loop over the rows of the first output which were reached, in ascending
order, per observable and lane. Every comparison is bit for bit (the NaN patterns as masks), and in every test state,
double-length times, propagate_res_arrays() and the Taylor coefficients of the two integrators are identical."""
import re
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

from test_grid_observables_gpu import (M, G, OC, _log_capture, assert_identical, collision_state, lane_grid, osc, outer_ss_obs,
                                       pendulum, pendulum_inputs, results, same, stop_after)

pytestmark = pytest.mark.gpu

ALL = ["min", "max", "t_min", "t_max", "sum", "last", "count"]


def grid_2d(grid, n):
    g = np.asarray(grid, dtype=float)
    return np.repeat(g[:, None], n, axis=1) if g.ndim == 1 else g


def fold(y, grid, stats=ALL):
    """(the statistics of y[point, observable, lane] as [observable, statistic, lane], the reached mask [point, lane]): a row
    which was not reached is NaN in every column, and the rows reached are a prefix of the grid of the lane."""
    n_grid, n_obs, n = y.shape
    g2 = grid_2d(grid, n)
    reached = ~np.isnan(y).all(axis=1)
    out = np.empty((n_obs, len(stats), n))
    for i in range(n):
        r = int(reached[:, i].sum())
        assert reached[:r, i].all()
        for o in range(n_obs):
            nan = float("nan")
            acc = dict(min=nan, max=nan, t_min=nan, t_max=nan, sum=nan, last=nan, count=0.0)
            for g in range(r):
                v, t = float(y[g, o, i]), float(g2[g, i])
                if g == 0:
                    acc = dict(min=v, max=v, t_min=t, t_max=t, sum=v, last=v, count=1.0)
                    continue
                if v < acc["min"] or acc["min"] != acc["min"]:
                    acc["min"], acc["t_min"] = v, t
                if v > acc["max"] or acc["max"] != acc["max"]:
                    acc["max"], acc["t_max"] = v, t
                acc["sum"] = acc["sum"] + v
                acc["last"] = v
                acc["count"] = acc["count"] + 1.0
            for k, s in enumerate(stats):
                out[o, k, i] = acc[s]
    return out, reached


def run_pair(make, obs, grid, stats=ALL, tas=None, make_cb=None, **kw):
    """(ta, tb, observable output, statistics, reached mask, the debug line of the run with statistics)."""
    ta, tb = tas if tas is not None else (make(), make())
    kwa, kwb = dict(kw), dict(kw)
    if make_cb is not None:
        kwa["callback"], kwb["callback"] = make_cb(), make_cb()
    with _log_capture() as la:
        _, y = ta.propagate_grid(grid, observables=obs, **kwa)
    with _log_capture() as lb:
        _, out = tb.propagate_grid(grid, observables=obs, statistics=stats, **kwb)
    assert out.shape == (len(obs), len(stats), y.shape[2])
    assert_identical(results(ta), results(tb))
    exp, reached = fold(y, grid, stats)
    bad = [(o, stats[k], i) for o, k, i in zip(*np.nonzero(~((out == exp) | (np.isnan(out) & np.isnan(exp)))))]
    print("[grid statistics] rows reached %d of %d, (observable, statistic, lane) which differ: %s" % (reached.sum(), reached.size, bad[:20]))
    assert same(out, exp), (out, exp)
    # The choice of the loop and its launches are those of the call with the observables alone.
    line_a, line_b = la.grid_lines()[0], lb.grid_lines()[0]
    assert line_b.startswith(line_a) and ", statistics " + ", ".join(stats) + " folded over the grid" in line_b[len(line_a):], (line_a, line_b)
    return ta, tb, y, out, reached, line_b


def stat(out, name, stats=ALL):
    return out[:, stats.index(name), :]


# ---- 1. the headline path ----
def test_headline_multi_step_launches_forward_backward_and_staged(monkeypatch):
    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=41)
    obs = outer_ss_obs(sys_)
    grid = lane_grid(n, 30.0, 13)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    ta, tb, _, out, reached, line = run_pair(make, obs, grid)
    assert "v5" in tb.hip_source_mode and reached.all()
    assert "multi-step launches" in line and "12 stepper launches for 12 grid intervals" in line, line
    assert "samples held in registers" in line and "(14 accumulators per system)" in line, line
    assert np.all(stat(out, "count") == 13.0)
    gb = grid[::-1].copy()
    _, _, _, outb, reached_b, _ = run_pair(None, obs, gb, tas=(ta, tb))
    assert reached_b.all()
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", "staged")
    tc = make()
    with _log_capture() as lc:
        _, out_s = tc.propagate_grid(grid, observables=obs, statistics=ALL)
        _, outb_s = tc.propagate_grid(gb, observables=obs, statistics=ALL)
    assert all("samples held in the staging buffer" in m and "multi-step launches" in m and "12 stepper launches" in m
               for m in lc.grid_lines())
    assert same(out_s, out) and same(outb_s, outb)
    assert_identical(results(tc), results(tb))


# ---- 2. a pendulum with parameters and time ----
@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_pendulum_batch_sizes_and_grid_kinds(n, ha):
    sys_, x, v, obs = pendulum()
    st, pars = pendulum_inputs(n)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, pars=pars, high_accuracy=ha)

    for grid in (lane_grid(n, 6.0, 7), np.linspace(0.0, 5.0, 5), np.array([0.0, 0.37]), lane_grid(n, 3.0, 4, backward=True)):
        *_, out, reached, line = run_pair(make, obs, grid)
        assert reached.all() and np.all(stat(out, "count") == len(grid))


def test_a_single_grid_point_is_row_zero():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    t0 = np.linspace(-1.0, 1.0, n)
    *_, y, out, reached, _ = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars, time=t0), obs, t0[None, :].copy())
    assert y.shape == (1, 1, n) and reached.all()
    for s in ("min", "max", "sum", "last"):
        assert same(stat(out, s), y[0])
    assert same(stat(out, "t_min")[0], t0) and same(stat(out, "t_max")[0], t0) and np.all(stat(out, "count") == 1.0)


# ---- 3. many points per step ----
def test_hundreds_of_points_inside_one_step():
    sys_, x, v, obs = pendulum()
    n = 3
    st, pars = pendulum_inputs(n)
    grid = np.linspace(0.0, 2.0, 2049)
    *_, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs + [x, x * v], grid)
    assert reached.all() and np.all(stat(out, "count") == 2049.0)
    assert int(re.search(r"(\d+) stepper launches for 2048 grid intervals", line).group(1)) < 100, line


# ---- 4. loops which end early ----
def test_max_steps_between_two_grid_points():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, _, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, grid, max_steps=9)
    assert "single-step sweeps" in line
    assert all(int(r[0]) == int(OC.step_limit) for r in tb.propagate_res)
    assert 1 < reached.all(axis=1).sum() < grid.shape[0]
    assert np.array_equal(stat(out, "count")[0], reached.sum(axis=0).astype(float))


def test_python_step_callback_which_stops_the_loop():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, _, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, grid,
                                            make_cb=lambda: stop_after(9))
    assert "single-step sweeps" in line and tb.last_callback_path == 1
    assert all(int(r[0]) == int(OC.cb_stop) for r in tb.propagate_res)
    assert 1 < reached.all(axis=1).sum() < grid.shape[0]
    assert np.array_equal(stat(out, "count")[0], reached.sum(axis=0).astype(float))


# ---- 5. a lane which goes non-finite ----
@pytest.mark.parametrize("semantics", [None, "per_lane"])
def test_nonfinite_lane_rollback_and_per_lane(semantics):
    """Default semantics: the launch with the non-finite lane is rolled back, the grid is redone in lock-step sweeps, and the
    sweep in which lane 1 goes non-finite un-samples what the other lanes took in it - the accumulators come back from their
    shadow copy. Behind row 1 the grid points of the lanes are spread so that every 0.01 of time holds one of some lane."""
    n = 67
    st = collision_state(n)
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    obs = outer_ss_obs(sys_)
    grid = np.empty((9, n))
    grid[0], grid[1] = 0.0, 0.3
    grid[2:] = 0.5 + 0.5 * np.arange(7)[:, None] + (0.5 / n) * np.arange(n)[None, :]
    ta, tb, y, out, reached, line = run_pair(
        lambda: hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, batch_semantics=semantics), obs, grid, max_delta_t=0.01)
    assert tb.propagate_res[1][0] == OC.err_nf_state
    assert ("rolled back to the start of the grid" in line) == (semantics is None), line
    assert reached[0].all() and reached[1].all() and not reached[-1].any()
    count = stat(out, "count")[0]
    assert np.array_equal(count, reached.sum(axis=0).astype(float))
    # The rows the grid index of a lane passed: those at or before the time the lane has reached.
    passed = (grid <= np.asarray(tb.time)[None, :]).sum(axis=0)
    others = np.arange(n) != 1
    print("[grid statistics] final times %s, lanes which lost rows: %s" % (np.unique(np.asarray(tb.time)[others]),
                                                                          np.nonzero(others & (count < passed))[0].tolist()))
    if semantics is None:
        assert np.any(count[others] < passed[others])


# ---- 6. independent semantics ----
@pytest.mark.parametrize("n", [5, 65])
def test_independent_semantics_retired_systems(n):
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), x * v]
    st = np.stack([np.zeros(n), np.linspace(0.8, 1.6, n)])
    grid = lane_grid(n, 9.0, 10)

    def make(s=st, m=n):
        return hy.taylor_adaptive_batch(sys_, s, m, t_events=[hy.t_event(x - 1.2)], batch_semantics="independent")

    ta, tb, y, out, reached, line = run_pair(make, obs, grid)
    retired = np.array([int(r[0]) == -1 for r in tb.propagate_res])
    assert tb.n_retired == retired.sum() and 0 < retired.sum() < n
    assert np.all(stat(out, "count")[0][~retired] == 10.0) and np.all(stat(out, "count")[0][retired] < 10.0)
    for i in range(n):
        t1 = make(st[:, i : i + 1].copy(), 1)
        _, o1 = t1.propagate_grid(grid[:, i : i + 1].copy(), observables=obs, statistics=ALL)
        assert same(o1[:, :, 0], out[:, :, i]), i


# ---- 7. other steppers ----
@pytest.mark.parametrize("emitter", [None, "table"])
def test_oscillator_unrolled_and_table_steppers(emitter):
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), hy.atan2(x, v), v]
    n = 5
    rng = np.random.RandomState(5)
    st = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])
    ta, tb, *_, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, emitter=emitter), obs, lane_grid(n, 7.0, 8))
    assert reached.all() and "(21 accumulators per system)" in line
    if emitter:
        assert "table" in tb.hip_source_mode


# ---- 8. contraction and NaN ----
def test_a_product_before_the_sum_and_nan_values():
    """x * v ends in a product: a sum contracted with it into an FMA differs in the last bit. log(x) and sqrt(v) are NaN over
    half of every period: minimum and maximum skip those rows, the sum keeps them."""
    sys_, x, v = osc()
    obs = [x * v, hy.log(x), hy.sqrt(v)]
    n = 65
    rng = np.random.RandomState(23)
    st = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])
    *_, y, out, reached, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n), obs, lane_grid(n, 7.0, 15))
    assert reached.all()
    nan = np.isnan(y[:, 1:, :])
    assert np.any(nan[1:-1] & ~nan[2:]) and np.any(nan[0] & ~nan[1:].all(axis=0))
    assert not np.isnan(y[:, 0, :]).any()
    # (What the rules say: an extremum is NaN only if every value is, a sum if any value is.)
    assert np.array_equal(np.isnan(stat(out, "min")[1:]), nan.all(axis=0)) and np.array_equal(np.isnan(stat(out, "sum")[1:]), nan.any(axis=0))


# ---- 9. a caller-owned device buffer ----
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
        _, out = ta.propagate_grid(grid, observables=obs, statistics=ALL)
        count = len(obs) * len(ALL) * n
        buf = torch.full((count + 4096,), sentinel, dtype=torch.float64, device="cuda")
        tb.propagate_grid_device(grid, buf.data_ptr(), observables=obs, statistics=ALL)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert same(host[:count].reshape(out.shape), out)
        assert not np.any(host[:count] == sentinel) and np.all(host[count:] == sentinel)
        assert_identical(results(ta), results(tb))


# ---- 10. run to run, batch size and position ----
def test_run_to_run_and_batch_independence():
    sys_, x, v, obs = pendulum()
    n = 65
    st, pars = pendulum_inputs(n, seed=13)
    grid = lane_grid(n, 6.0, 7)

    def run(idx):
        idx = np.asarray(idx)
        ta = hy.taylor_adaptive_batch(sys_, st[:, idx].copy(), len(idx), pars=pars[:, idx].copy(), high_accuracy=True)
        return ta.propagate_grid(grid[:, idx].copy(), observables=obs, statistics=ALL)[1]

    a, b = run(np.arange(n)), run(np.arange(n))
    assert same(a, b) and not np.isnan(a).any()
    for idx in ([64], [7], [3, 64, 7], list(reversed(range(n)))):
        o = run(idx)
        assert same(o, a[:, :, idx]), idx


# ---- 11. the C++ program ----
def test_cpp_grid_statistics_on_gpu():
    from test_grid_statistics import build_cpp

    out = subprocess.run([build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
