"""Ensemble statistics on the MI355X. The yardstick is what exists without the feature: the same integrator
built twice, one runs ``propagate_grid(grid, observables=obs)`` and the other adds ``ensemble_statistics=``; the expected
values are the reference in rational arithmetic of tests/test_grid_ensemble.py applied to the output Y of the first, per grid
row and observable over the lanes. Every comparison is bit for bit (the NaN patterns as masks), the words of the accumulators
are those the host twin of the kernel makes of Y, and in every test state, double-length times, propagate_res_arrays() and the
Taylor coefficients of the two integrators are identical."""
import re
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

from test_grid_ensemble import ADVERSARIAL, ALL, random_doubles, ref_fold, same
from test_grid_observables_gpu import (M, G, OC, _log_capture, assert_identical, collision_state, lane_grid, osc, outer_ss_obs,
                                       pendulum, pendulum_inputs, results, stop_after)

pytestmark = pytest.mark.gpu


def host_words(y, stats):
    """The accumulators the host twin of the kernel makes of y[point, observable, lane]."""
    acc = hy.ensemble_accumulators(y.shape[0], y.shape[1], stats)
    for g in range(y.shape[0]):
        for o in range(y.shape[1]):
            for v in y[g, o]:
                acc.add(g, o, v)
    return acc.raw


def run_pair(make, obs, grid, stats=ALL, tas=None, make_cb=None, **kw):
    """(ta, tb, observable output, accumulators, the debug line of the run with the ensemble statistics)."""
    ta, tb = tas if tas is not None else (make(), make())
    kwa, kwb = dict(kw), dict(kw)
    if make_cb is not None:
        kwa["callback"], kwb["callback"] = make_cb(), make_cb()
    with _log_capture() as la:
        _, y = ta.propagate_grid(grid, observables=obs, **kwa)
    with _log_capture() as lb:
        _, acc = tb.propagate_grid(grid, observables=obs, ensemble_statistics=stats, **kwb)
    out = acc.values
    assert out.shape == (y.shape[0], len(obs), len(stats))
    assert_identical(results(ta), results(tb))
    exp = ref_fold(y, stats)
    bad = [(g, o, stats[k]) for g, o, k in zip(*np.nonzero(~((out == exp) | (np.isnan(out) & np.isnan(exp)))))]
    print("[grid ensemble] %d lanes, non-NaN entries %d of %d, (row, observable, statistic) which differ: %s"
          % (y.shape[2], (~np.isnan(y)).sum(), y.size, bad[:20]))
    assert same(out, exp), (out, exp)
    assert np.array_equal(acc.raw, host_words(y, stats))
    # The choice of the loop and its launches are those of the call with the observables alone.
    line_a, line_b = la.grid_lines()[0], lb.grid_lines()[0]
    assert line_b.startswith(line_a) and ", ensemble statistics merged across the systems per grid point (" in line_b[len(line_a):], (line_a, line_b)
    return ta, tb, y, acc, line_b


def stat(acc, name, stats=ALL):
    return acc.values[:, :, stats.index(name)]


# ---- 1. the headline path ----
def test_headline_multi_step_launches_forward_backward_and_staged(monkeypatch):
    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=41)
    obs = outer_ss_obs(sys_)
    grid = lane_grid(n, 30.0, 13)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    ta, tb, _, acc, line = run_pair(make, obs, grid)
    assert "v5" in tb.hip_source_mode
    assert "multi-step launches" in line and "12 stepper launches for 12 grid intervals" in line, line
    assert "samples held in registers" in line and "(139 words per grid point and observable, aggregated per wavefront)" in line, line
    assert np.all(stat(acc, "count") == float(n))
    gb = grid[::-1].copy()
    _, _, _, accb, _ = run_pair(None, obs, gb, tas=(ta, tb))
    assert np.all(stat(accb, "count") == float(n))
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", "staged")
    tc = make()
    with _log_capture() as lc:
        _, acc_s = tc.propagate_grid(grid, observables=obs, ensemble_statistics=ALL)
        _, accb_s = tc.propagate_grid(gb, observables=obs, ensemble_statistics=ALL)
    assert all("samples held in the staging buffer" in m and "multi-step launches" in m and "12 stepper launches" in m
               for m in lc.grid_lines())
    assert np.array_equal(acc_s.raw, acc.raw) and np.array_equal(accb_s.raw, accb.raw)
    assert_identical(results(tc), results(tb))


# ---- 2. the smallest shapes: one lane, a ragged wavefront, a full one, one lane into the next, into a second workgroup ----
@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_pendulum_batch_sizes_and_grid_kinds(n):
    sys_, x, v, obs = pendulum()
    obs = obs + [hy.gt(x, 0.0), x * v]
    st, pars = pendulum_inputs(n)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, pars=pars, high_accuracy=bool(n % 2))

    for grid in (lane_grid(n, 6.0, 7), np.linspace(0.0, 5.0, 5), np.array([0.0, 0.37]), lane_grid(n, 3.0, 4, backward=True)):
        *_, y, acc, line = run_pair(make, obs, grid)
        assert np.all(stat(acc, "count") == float(n))
        # (A comparison is 0 or 1: its sum counts the systems which satisfy it.)
        assert np.array_equal(stat(acc, "sum")[:, 1], (y[:, 1, :] == 1.0).sum(axis=1).astype(float))


def test_a_single_grid_point_is_row_zero():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    t0 = np.linspace(-1.0, 1.0, n)
    *_, y, acc, _ = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars, time=t0), obs, t0[None, :].copy())
    assert y.shape == (1, 1, n) and acc.values.shape == (1, 1, len(ALL)) and stat(acc, "count")[0, 0] == n
    assert stat(acc, "min")[0, 0] == y.min() and stat(acc, "max")[0, 0] == y.max()


# ---- 3. many points per step: a lane crosses several rows in one launch ----
def test_hundreds_of_points_inside_one_step():
    sys_, x, v, obs = pendulum()
    n = 3
    st, pars = pendulum_inputs(n)
    grid = np.linspace(0.0, 2.0, 2049)
    *_, acc, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs + [x, x * v], grid,
                             stats=["count", "min", "mean"])
    assert np.all(stat(acc, "count", ["count", "min", "mean"]) == 3.0)
    assert int(re.search(r"(\d+) stepper launches for 2048 grid intervals", line).group(1)) < 100, line


# ---- 4. adversarial values: the parameters are the observables ----
def par_system():
    """An oscillator whose parameters do not move it: par[0] and par[1] only choose between two finite rates of w."""
    x, v, w = hy.make_vars("x", "v", "w")
    return [(x, v), (v, -x), (w, 0.5 + hy.gt(hy.par[0], hy.par[1]))], [hy.par[0], hy.par[0] * hy.par[1]]


def run_pars(p0, p1, grid=(0.0, 0.4, 0.9)):
    sys_, obs = par_system()
    n = len(p0)
    st = np.stack([np.linspace(0.5, 1.5, n), np.zeros(n), np.zeros(n)])
    pars = np.stack([np.asarray(p0, dtype=float), np.asarray(p1, dtype=float)])
    ta, tb, y, acc, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, np.asarray(grid))
    assert all(int(r[0]) == int(OC.time_limit) for r in tb.propagate_res)
    # (The observables are the parameters, bit for bit, and one rounded product.)
    for g in range(y.shape[0]):
        assert same(y[g, 0], pars[0])
        with np.errstate(all="ignore"):
            assert same(y[g, 1], pars[0] * pars[1])
    return acc


@pytest.mark.parametrize("name", [k for k, v in ADVERSARIAL.items() if len(v)])
def test_adversarial_lists_as_parameters(name):
    vals = np.asarray(ADVERSARIAL[name], dtype=float)
    # The second observable squares the value once more in another order of magnitudes: p1 cycles over a few scales.
    p1 = np.array([1.0, -2.0**-30, 2.0**600, 3.0, -2.0**-700])[np.arange(len(vals)) % 5]
    run_pars(vals, p1)


def test_exponents_which_differ_inside_a_wavefront():
    """Every lane of the four wavefronts (and of the lane behind them) has another exponent and sign: the ballot loop takes as
    many turns as there are distinct first bins, and the sums still are the exact ones. Then blocks of equal exponents."""
    n = 257
    p0 = random_doubles(n, 77)
    p1 = random_doubles(n, 78)
    p1 = np.where(np.abs(np.log2(np.abs(p1) + 2.0**-1074)) > 300, 1.5, p1)  # (most products finite, some huge or tiny)
    run_pars(p0, p1)
    blocks = np.repeat(np.array([1.0, -2.0**40, 2.0**-1060, 2.0**1000]), 65)[:n] * (1.0 + np.arange(n) / 1024.0)
    blocks[[5, 70, 256]] = [np.nan, np.inf, -0.0]
    run_pars(blocks, np.full(n, 0.75))


# ---- 5. loops which end early: the count falls along the grid ----
def test_max_steps_between_two_grid_points():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, y, acc, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, grid, max_steps=9)
    assert "single-step sweeps" in line
    assert all(int(r[0]) == int(OC.step_limit) for r in tb.propagate_res)
    count = stat(acc, "count")[:, 0]
    assert count[0] == n and count[-1] == 0 and np.all(np.diff(count) <= 0) and np.array_equal(count, (~np.isnan(y[:, 0])).sum(axis=1))
    assert np.isnan(stat(acc, "min")[-1, 0]) and stat(acc, "sum")[-1, 0] == 0.0


def test_python_step_callback_which_stops_the_loop():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, y, acc, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, grid,
                                    make_cb=lambda: stop_after(9))
    assert "single-step sweeps" in line and tb.last_callback_path == 1
    assert all(int(r[0]) == int(OC.cb_stop) for r in tb.propagate_res)
    count = stat(acc, "count")[:, 0]
    assert count[0] == n and count[-1] == 0 and np.all(np.diff(count) <= 0)


# ---- 6. a lane which goes non-finite: the rollback of the launches, and the restore of the records in a lock-step sweep ----
@pytest.mark.parametrize("semantics", [None, "per_lane"])
def test_nonfinite_lane_rollback_and_per_lane(semantics):
    n = 67
    st = collision_state(n)
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    obs = outer_ss_obs(sys_)
    grid = np.empty((9, n))
    grid[0], grid[1] = 0.0, 0.3
    grid[2:] = 0.5 + 0.5 * np.arange(7)[:, None] + (0.5 / n) * np.arange(n)[None, :]
    ta, tb, y, acc, line = run_pair(
        lambda: hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, batch_semantics=semantics), obs, grid, max_delta_t=0.01)
    assert tb.propagate_res[1][0] == OC.err_nf_state
    assert ("rolled back to the start of the grid" in line) == (semantics is None), line
    count = stat(acc, "count")[:, 0]
    assert count[0] == n and count[1] == n and count[-1] == 0
    # The rows the grid index of a lane passed: those at or before the time the lane has reached. With the reference's
    # semantics the sweep in which lane 1 went non-finite took its samples back: some lane lost a row it had passed.
    passed = (grid <= np.asarray(tb.time)[None, :])
    others = np.arange(n) != 1
    if semantics is None:
        assert np.any(passed[:, others] & np.isnan(y[:, 0, :][:, others]))


# ---- 7. independent semantics ----
def test_independent_semantics_retired_systems_against_every_system_alone():
    n = 65
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), x * v]
    st = np.stack([np.zeros(n), np.linspace(0.8, 1.6, n)])
    grid = lane_grid(n, 9.0, 10)

    def make(s=st, m=n):
        return hy.taylor_adaptive_batch(sys_, s, m, t_events=[hy.t_event(x - 1.2)], batch_semantics="independent")

    ta, tb, y, acc, line = run_pair(make, obs, grid)
    retired = np.array([int(r[0]) == -1 for r in tb.propagate_res])
    assert tb.n_retired == retired.sum() and 0 < retired.sum() < n
    count = stat(acc, "count")[:, 0]
    assert count[0] == n and count[-1] == n - retired.sum()
    alone = hy.ensemble_accumulators(grid.shape[0], len(obs), ALL)
    for i in range(n):
        t1 = make(st[:, i : i + 1].copy(), 1)
        alone.merge(t1.propagate_grid(grid[:, i : i + 1].copy(), observables=obs, ensemble_statistics=ALL)[1])
    assert np.array_equal(alone.raw, acc.raw)


# ---- 8. other steppers ----
@pytest.mark.parametrize("emitter", [None, "table"])
def test_oscillator_unrolled_and_table_steppers(emitter):
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), hy.log(x), v]
    n = 67
    rng = np.random.RandomState(5)
    st = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])
    ta, tb, y, acc, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, emitter=emitter), obs, lane_grid(n, 7.0, 8))
    if emitter:
        assert "table" in tb.hip_source_mode
    # log(x) is NaN over half of every period: those values are skipped, the count says how many were.
    nan = np.isnan(y[:, 1, :])
    assert nan.any() and not nan.all(axis=1).any() and np.array_equal(stat(acc, "count")[:, 1], (~nan).sum(axis=1))


# ---- 9. sharding, the switch, run to run, batch position ----
def shard_setup():
    sys_, x, v, obs = pendulum()
    n = 130
    st, pars = pendulum_inputs(n, seed=13)
    grid = lane_grid(n, 6.0, 7)

    def run(idx):
        idx = np.asarray(idx)
        ta = hy.taylor_adaptive_batch(sys_, st[:, idx].copy(), len(idx), pars=pars[:, idx].copy(), high_accuracy=True)
        return ta.propagate_grid(grid[:, idx].copy(), observables=obs + [x * v], ensemble_statistics=ALL)[1]

    return n, run


def test_one_batch_and_its_shards_merge_to_identical_words(monkeypatch):
    monkeypatch.delenv("HEYOKA_AMD_GRID_ENS", raising=False)
    n, run = shard_setup()
    whole = run(np.arange(n))
    assert np.all(stat(whole, "count") == float(n))
    # Run to run.
    assert np.array_equal(run(np.arange(n)).raw, whole.raw)
    # Shards of 65 + 64 + 1, merged in two orders.
    a, b, c = run(np.arange(65)), run(np.arange(65, 129)), run([129])
    m1 = run(np.arange(65)).merge(b).merge(c)
    m2 = run([129]).merge(a).merge(b)
    assert np.array_equal(m1.raw, whole.raw) and np.array_equal(m2.raw, whole.raw) and same(m1.values, whole.values)
    # Batch position: a permutation of the lanes.
    perm = np.random.RandomState(3).permutation(n)
    assert np.array_equal(run(perm).raw, whole.raw) and np.array_equal(run(np.arange(n)[::-1]).raw, whole.raw)
    # One atomic per lane and word instead of the aggregation per wavefront: the same words.
    monkeypatch.setenv("HEYOKA_AMD_GRID_ENS", "peratomic")
    with _log_capture() as lc:
        per = run(np.arange(n))
    assert "one atomic per lane" in lc.grid_lines()[0]
    assert np.array_equal(per.raw, whole.raw)


def test_peratomic_on_adversarial_values(monkeypatch):
    monkeypatch.setenv("HEYOKA_AMD_GRID_ENS", "peratomic")
    n = 130
    run_pars(random_doubles(n, 5), np.where(np.arange(n) % 3 == 0, 2.0**500, 0.5))


# ---- 10. a caller-owned device buffer ----
def test_device_buffer_words_and_extent():
    import torch

    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=48)
    obs = outer_ss_obs(sys_)
    sentinel = -1234567

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    for grid in (lane_grid(n, 10.0, 6), np.linspace(0.0, 8.0, 5)):
        ta, tb = make(), make()
        _, acc = ta.propagate_grid(grid, observables=obs, ensemble_statistics=ALL)
        count = acc.raw.size
        buf = torch.full((count + 4096,), sentinel, dtype=torch.int64, device="cuda")
        tb.propagate_grid_device(grid, buf.data_ptr(), observables=obs, ensemble_statistics=ALL)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[:count].view(np.uint64), acc.raw)
        assert np.all(host[count:] == sentinel)
        assert_identical(results(ta), results(tb))


# ---- 11. the C++ program ----
def test_cpp_grid_ensemble_on_gpu():
    from test_grid_ensemble import build_cpp

    out = subprocess.run([build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
