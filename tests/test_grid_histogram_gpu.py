"""Ensemble histograms on the MI355X. The yardstick is what exists without the feature: the same integrator built
twice, one runs ``propagate_grid(grid, observables=obs)`` and the other adds ``ensemble_histograms=``; the expected counters are
``numpy.searchsorted(edges, ., side="right")`` plus a NaN filter and a bincount (ref_counts() of tests/test_grid_histogram.py)
applied to the output Y of the first, per grid row and observable over the lanes. Every counter is compared as an integer, and
in every test state, double-length times, propagate_res_arrays() and the Taylor coefficients of the two integrators are
identical."""
import re
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs

from test_grid_histogram import MODES, ref_counts
from test_grid_observables_gpu import (M, G, OC, _log_capture, assert_identical, collision_state, lane_grid, osc, outer_ss_obs,
                                       pendulum, pendulum_inputs, results, stop_after)

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
PENDULUM_EDGES = np.linspace(-11.0, -1.0, 9)  # (8 bins over the energies of pendulum_inputs(), some of which lie outside)


def expected_raw(edges, y):
    """The counters of y[point, observable, lane] in the layout of the records: (n_grid, W)."""
    return np.concatenate([ref_counts(e, y[:, o, :]) for o, e in enumerate(edges) if e is not None and len(e)], axis=1)


def check_hist(hist, edges, y):
    exp = expected_raw(edges, y)
    got = hist.raw.reshape(exp.shape)
    bad = np.argwhere(got != exp)
    print("[grid histogram] %d lanes, non-NaN entries %d of %d, total counted %d, (row, word) which differ: %s"
          % (y.shape[2], (~np.isnan(y)).sum(), y.size, got.sum(), bad[:20].tolist()))
    assert hist.raw.dtype == np.uint64 and np.array_equal(got, exp)
    for o, e in enumerate(edges):
        if e is not None and len(e):
            assert np.array_equal(hist.counts(o), ref_counts(e, y[:, o, :]))
            assert np.array_equal(hist.counts(o).sum(axis=1), (~np.isnan(y[:, o, :])).sum(axis=1))


def run_pair(make, obs, grid, edges, tas=None, make_cb=None, **kw):
    """(ta, tb, observable output, histograms, the debug line of the run with the histograms). edges: the lists, or a function
    of the observable output which makes them - the edges are data of the call."""
    ta, tb = tas if tas is not None else (make(), make())
    kwa, kwb = dict(kw), dict(kw)
    if make_cb is not None:
        kwa["callback"], kwb["callback"] = make_cb(), make_cb()
    with _log_capture() as la:
        _, y = ta.propagate_grid(grid, observables=obs, **kwa)
    if callable(edges):
        edges = edges(y)
    with _log_capture() as lb:
        _, hist = tb.propagate_grid(grid, observables=obs, ensemble_histograms=edges, **kwb)
    assert_identical(results(ta), results(tb))
    check_hist(hist, edges, y)
    # The choice of the loop and its launches are those of the call with the observables alone.
    line_a, line_b = la.grid_lines()[0], lb.grid_lines()[0]
    tail = line_b[len(line_a):]
    assert line_b.startswith(line_a) and ", ensemble histograms counted across the systems per grid point (" in tail, (line_a, line_b)
    assert "%d words per grid point, merge mode " % hist.words in tail, tail
    return ta, tb, y, hist, line_b


def outer_ss_edges(y):
    """256 bins over the energies of the first row - the largest one is the last edge: the overflow slot -, 256 over most of the
    squared distances."""
    return [np.linspace(y[0, 0].min(), y[0, 0].max(), 257), np.linspace(y[:, 1].min() * 0.9, y[:, 1].max() * 0.95, 257)]


# ---- 1. the headline path ----
def test_headline_multi_step_launches_forward_backward_and_staged(monkeypatch):
    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=41)
    obs = outer_ss_obs(sys_)
    grid = lane_grid(n, 30.0, 13)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    ta, tb, y, hist, line = run_pair(make, obs, grid, outer_ss_edges)
    assert "v5" in tb.hip_source_mode
    assert "multi-step launches" in line and "12 stepper launches for 12 grid intervals" in line, line
    assert "samples held in registers" in line and re.search(r"\(516 words per grid point, merge mode hybrid of [124] turns\)", line), line
    assert np.all(hist.counts(0).sum(axis=1) == n) and np.all(hist.counts(1).sum(axis=1) == n)
    assert hist.counts(1)[:, -1].sum() > 0  # (some distances beyond the last edge)
    edges = hist.edges
    gb = grid[::-1].copy()
    _, _, _, histb, _ = run_pair(None, obs, gb, edges, tas=(ta, tb))
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", "staged")
    tc = make()
    with _log_capture() as lc:
        _, hist_s = tc.propagate_grid(grid, observables=obs, ensemble_histograms=edges)
        _, histb_s = tc.propagate_grid(gb, observables=obs, ensemble_histograms=edges)
    assert all("samples held in the staging buffer" in m and "multi-step launches" in m and "12 stepper launches" in m
               for m in lc.grid_lines())
    assert np.array_equal(hist_s.raw, hist.raw) and np.array_equal(histb_s.raw, histb.raw)
    assert_identical(results(tc), results(tb))


# ---- 2. the smallest shapes: one lane, a ragged wavefront, a full one, one lane into the next, into a second workgroup ----
@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_pendulum_batch_sizes_and_grid_kinds(n):
    sys_, x, v, obs = pendulum()
    obs = obs + [x * v]
    st, pars = pendulum_inputs(n)
    edges = [PENDULUM_EDGES, np.linspace(-1.0, 1.0, 9)]

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, pars=pars, high_accuracy=bool(n % 2))

    for grid in (lane_grid(n, 6.0, 7), np.linspace(0.0, 5.0, 5), np.array([0.0, 0.37]), lane_grid(n, 3.0, 4, backward=True)):
        *_, hist, line = run_pair(make, obs, grid, edges)
        assert hist.words == 20 and np.all(hist.counts(0).sum(axis=1) == n)


def test_a_single_grid_point_is_row_zero():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    t0 = np.linspace(-1.0, 1.0, n)
    *_, y, hist, _ = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars, time=t0), obs, t0[None, :].copy(),
                              [PENDULUM_EDGES])
    assert y.shape == (1, 1, n) and hist.counts(0).shape == (1, 10) and hist.counts(0).sum() == n


# ---- 3. many points per step: a lane crosses several rows in one launch ----
def test_hundreds_of_points_inside_one_step():
    sys_, x, v, obs = pendulum()
    n = 3
    st, pars = pendulum_inputs(n)
    grid = np.linspace(0.0, 2.0, 2049)
    *_, hist, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs + [x, x * v], grid,
                              [PENDULUM_EDGES, None, np.linspace(-2.0, 2.0, 9)])
    assert np.all(hist.counts(0).sum(axis=1) == 3) and np.all(hist.counts(2).sum(axis=1) == 3)
    assert int(re.search(r"(\d+) stepper launches for 2048 grid intervals", line).group(1)) < 100, line


# ---- 4. adversarial values: the parameter is the observable ----
def par_system():
    """An oscillator whose parameter does not move it: par[0] only chooses between two finite rates of w."""
    x, v, w = hy.make_vars("x", "v", "w")
    return [(x, v), (v, -x), (w, 0.5 + hy.gt(hy.par[0], 0.25))], [hy.par[0]]


B256 = np.arange(257.0)  # (256 bins [k, k + 1))


def par_lists():
    n = 257
    spread = np.arange(n) - 0.5  # (lane k in slot k: the underflow slot and every bin, nobody in the overflow)
    blocks = np.repeat(np.array([3.5, 3.75, 100.0, 255.5]), 65)[:n].copy()
    blocks[[5, 70, 140, 256]] = [NAN, INF, -INF, -0.0]
    return {
        "spread": spread,
        "concentrated": np.full(n, 17.25),
        "overflow": np.full(n, 1e300),
        "blocks": blocks,
        "mixed": np.where(np.arange(n) % 3 == 0, 17.25, spread),
    }


def run_pars(p0, edges=B256, grid=(0.0, 0.4, 0.9)):
    sys_, obs = par_system()
    n = len(p0)
    st = np.stack([np.linspace(0.5, 1.5, n), np.zeros(n), np.zeros(n)])
    pars = np.asarray(p0, dtype=float)[None, :].copy()
    ta, tb, y, hist, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, np.asarray(grid), [edges])
    assert all(int(r[0]) == int(OC.time_limit) for r in tb.propagate_res)
    for g in range(y.shape[0]):
        assert np.array_equal(y[g, 0].view(np.uint64), pars[0].view(np.uint64))
    return hist


@pytest.mark.parametrize("name", ["spread", "concentrated", "overflow", "blocks"])
def test_adversarial_lists_as_parameters(name):
    hist = run_pars(par_lists()[name])
    c = hist.counts(0)
    if name == "spread":
        assert np.all(c[:, :257] == 1) and np.all(c[:, 257] == 0)
    elif name == "concentrated":
        assert np.all(c[:, 18] == 257) and c.sum() == 3 * 257
    elif name == "overflow":
        assert np.all(c[:, 257] == 257) and c.sum() == 3 * 257
    else:
        # (-inf: the underflow slot; -0.0 compares equal to the edge 0.0 and is in bin 1 like +0.0; +inf: the overflow slot; the
        # NaN is not counted.)
        assert np.all(c.sum(axis=1) == 256) and np.all(c[:, 0] == 1) and np.all(c[:, 1] == 1) and np.all(c[:, 257] == 1)


def test_4096_bins_values_on_the_edges_and_beside_them():
    """The 13-step search over 4 097 edges on the device: values equal to some 230 of the edges - the first, the last, and edges
    on both sides of every stride of the search - and the doubles next to them on either side, a lane each."""
    edges = np.linspace(-3.0, 5.0, 4097)
    e = edges[np.unique(np.concatenate([np.linspace(0, 4096, 200).astype(int), 2 ** np.arange(13), 2 ** np.arange(13) - 1,
                                        4096 - 2 ** np.arange(12)]))][:257]
    vals = np.concatenate([e, np.nextafter(e, -INF), np.nextafter(e, INF)])
    hist = run_pars(vals, edges=edges)
    c = hist.counts(0)
    assert c.shape == (3, 4098) and np.all(c.sum(axis=1) == vals.size) and c[0, 0] == 1 and c[0, 4097] == 2


@pytest.mark.parametrize("name", ["spread", "concentrated", "mixed"])
def test_the_three_merge_modes_give_identical_words(name, monkeypatch):
    raws = []
    monkeypatch.delenv("HEYOKA_AMD_GRID_HIST_TURNS", raising=False)
    for mode in MODES:
        monkeypatch.setenv("HEYOKA_AMD_GRID_HIST", mode)
        with _log_capture() as lc:
            raws.append(run_pars(par_lists()[name]).raw)
        assert all("merge mode %s" % mode in m for m in lc.grid_lines() if "histograms" in m)
    # ... and every number of turns of the hybrid mode which was measured.
    monkeypatch.setenv("HEYOKA_AMD_GRID_HIST", "hybrid")
    for k in (1, 2, 4):
        monkeypatch.setenv("HEYOKA_AMD_GRID_HIST_TURNS", str(k))
        with _log_capture() as lc:
            raws.append(run_pars(par_lists()[name]).raw)
        assert all("merge mode hybrid of %d turns)" % k in m for m in lc.grid_lines() if "histograms" in m)
    assert all(np.array_equal(raws[0], r) for r in raws[1:]) and raws[0].sum() == 3 * 257


# ---- 5. loops which end early: the total count falls along the grid ----
def test_max_steps_between_two_grid_points():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, y, hist, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, grid, [PENDULUM_EDGES], max_steps=9)
    assert "single-step sweeps" in line
    assert all(int(r[0]) == int(OC.step_limit) for r in tb.propagate_res)
    count = hist.counts(0).sum(axis=1)
    assert count[0] == n and count[-1] == 0 and np.all(np.diff(count.astype(np.int64)) <= 0)


def test_python_step_callback_which_stops_the_loop():
    sys_, x, v, obs = pendulum()
    n = 5
    st, pars = pendulum_inputs(n)
    grid = lane_grid(n, 2.0, 9)
    ta, tb, y, hist, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, pars=pars), obs, grid, [PENDULUM_EDGES],
                                     make_cb=lambda: stop_after(9))
    assert "single-step sweeps" in line and tb.last_callback_path == 1
    assert all(int(r[0]) == int(OC.cb_stop) for r in tb.propagate_res)
    count = hist.counts(0).sum(axis=1)
    assert count[0] == n and count[-1] == 0 and np.all(np.diff(count.astype(np.int64)) <= 0)


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

    def edges(y):
        fin = y[:, 1][np.isfinite(y[:, 1])]
        return [None, np.linspace(fin.min(), fin.max(), 33)]

    ta, tb, y, hist, line = run_pair(
        lambda: hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, batch_semantics=semantics), obs, grid, edges,
        max_delta_t=0.01)
    assert tb.propagate_res[1][0] == OC.err_nf_state
    assert ("rolled back to the start of the grid" in line) == (semantics is None), line
    count = hist.counts(1).sum(axis=1)
    assert count[0] == n and count[1] == n and count[-1] == 0
    passed = (grid <= np.asarray(tb.time)[None, :])
    others = np.arange(n) != 1
    if semantics is None:
        # (The sweep in which lane 1 went non-finite took its samples back: the records were restored from their copy.)
        assert np.any(passed[:, others] & np.isnan(y[:, 0, :][:, others]))


# ---- 7. independent semantics ----
def test_independent_semantics_retired_systems_against_every_system_alone():
    n = 65
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), x * v]
    st = np.stack([np.zeros(n), np.linspace(0.8, 1.6, n)])
    grid = lane_grid(n, 9.0, 10)
    edges = [np.linspace(0.3, 1.3, 9), np.linspace(-0.6, 0.6, 9)]

    def make(s=st, m=n):
        return hy.taylor_adaptive_batch(sys_, s, m, t_events=[hy.t_event(x - 1.2)], batch_semantics="independent")

    ta, tb, y, hist, line = run_pair(make, obs, grid, edges)
    retired = np.array([int(r[0]) == -1 for r in tb.propagate_res])
    assert tb.n_retired == retired.sum() and 0 < retired.sum() < n
    count = hist.counts(0).sum(axis=1)
    assert count[0] == n and count[-1] == n - retired.sum()
    alone = hy.ensemble_histogram_accumulators(grid.shape[0], edges)
    for i in range(n):
        t1 = make(st[:, i : i + 1].copy(), 1)
        alone.merge(t1.propagate_grid(grid[:, i : i + 1].copy(), observables=obs, ensemble_histograms=edges)[1])
    assert np.array_equal(alone.raw, hist.raw)


# ---- 8. other steppers ----
@pytest.mark.parametrize("emitter", [None, "table"])
def test_oscillator_unrolled_and_table_steppers(emitter):
    sys_, x, v = osc()
    obs = [0.5 * (x * x + v * v), hy.log(x), v]
    n = 67
    rng = np.random.RandomState(5)
    st = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.5, 0.5, n)])
    edges = [None, np.linspace(-3.0, 0.5, 9), np.linspace(-1.0, 1.0, 5)]
    ta, tb, y, hist, line = run_pair(lambda: hy.taylor_adaptive_batch(sys_, st, n, emitter=emitter), obs, lane_grid(n, 7.0, 8), edges)
    if emitter:
        assert "table" in tb.hip_source_mode
    # log(x) is NaN over half of every period: those values are skipped, the total says how many were.
    nan = np.isnan(y[:, 1, :])
    assert nan.any() and not nan.all(axis=1).any() and np.array_equal(hist.counts(1).sum(axis=1), (~nan).sum(axis=1))


# ---- 9. sharding, run to run, batch position ----
def test_one_batch_and_its_shards_merge_to_identical_words(monkeypatch):
    monkeypatch.delenv("HEYOKA_AMD_GRID_HIST", raising=False)
    sys_, x, v, obs = pendulum()
    n = 130
    st, pars = pendulum_inputs(n, seed=13)
    grid = lane_grid(n, 6.0, 7)
    edges = [PENDULUM_EDGES, np.linspace(-1.0, 1.0, 33)]

    def run(idx):
        idx = np.asarray(idx)
        ta = hy.taylor_adaptive_batch(sys_, st[:, idx].copy(), len(idx), pars=pars[:, idx].copy(), high_accuracy=True)
        return ta.propagate_grid(grid[:, idx].copy(), observables=obs + [x * v], ensemble_histograms=edges)[1]

    whole = run(np.arange(n))
    assert np.all(whole.counts(0).sum(axis=1) == n)
    assert np.array_equal(run(np.arange(n)).raw, whole.raw)
    a, b, c = run(np.arange(65)), run(np.arange(65, 129)), run([129])
    m1 = run(np.arange(65)).merge(b).merge(c)
    m2 = run([129]).merge(a).merge(b)
    assert np.array_equal(m1.raw, whole.raw) and np.array_equal(m2.raw, whole.raw)
    perm = np.random.RandomState(3).permutation(n)
    assert np.array_equal(run(perm).raw, whole.raw) and np.array_equal(run(np.arange(n)[::-1]).raw, whole.raw)


# ---- 10. together with the ensemble statistics ----
def test_combined_with_ensemble_statistics():
    stats = ["count", "mean", "min", "max", "sum_sq"]
    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=43)
    obs = outer_ss_obs(sys_)
    grid = lane_grid(n, 20.0, 9)

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    ta, tb, y, hist, _ = run_pair(make, obs, grid, outer_ss_edges)
    tc, td = make(), make()
    _, acc = tc.propagate_grid(grid, observables=obs, ensemble_statistics=stats)
    with _log_capture() as lc:
        _, (acc2, hist2) = td.propagate_grid(grid, observables=obs, ensemble_statistics=stats, ensemble_histograms=hist.edges)
    line = lc.grid_lines()[0]
    assert ", ensemble statistics merged across the systems per grid point (" in line and ", ensemble histograms counted" in line
    assert np.array_equal(acc2.raw, acc.raw) and np.array_equal(hist2.raw, hist.raw)
    assert_identical(results(td), results(ta))
    for o in range(2):
        assert np.array_equal(hist2.counts(o).sum(axis=1).astype(float), acc2.values[:, o, 0])
    # One histogram only, in single-step sweeps (max_steps): the shadow copy covers both regions.
    te, tf = make(), make()
    _, y2 = te.propagate_grid(grid, observables=obs, max_steps=7)
    _, (acc3, hist3) = tf.propagate_grid(grid, observables=obs, ensemble_statistics=["count"], max_steps=7,
                                         ensemble_histograms=[None, hist.edges[1]])
    check_hist(hist3, [None, hist.edges[1]], y2)
    assert np.array_equal(acc3.values[:, 1, 0], hist3.counts(1).sum(axis=1).astype(float)) and acc3.values[-1, 1, 0] == 0


# ---- 11. a caller-owned device buffer ----
@pytest.mark.parametrize("stats", [None, ["count", "mean"]])
def test_device_buffer_words_and_guards(stats):
    import torch

    n = 67
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=48)
    obs = outer_ss_obs(sys_)
    sentinel = -1234567
    guard = 4096

    def make():
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)

    edges = None
    for grid in (lane_grid(n, 10.0, 6), np.linspace(0.0, 8.0, 5)):
        ta, tb = make(), make()
        if edges is None:
            edges = outer_ss_edges(ta.propagate_grid(grid, observables=obs)[1])
            ta = make()
        _, ret = ta.propagate_grid(grid, observables=obs, ensemble_statistics=stats, ensemble_histograms=edges)
        words = ret.raw if stats is None else np.concatenate([ret[0].raw, ret[1].raw])
        count = words.size
        buf = torch.full((guard + count + guard,), sentinel, dtype=torch.int64, device="cuda")
        tb.propagate_grid_device(grid, buf.data_ptr() + 8 * guard, observables=obs, ensemble_statistics=stats,
                                 ensemble_histograms=edges)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[guard : guard + count].view(np.uint64), words)
        assert np.all(host[:guard] == sentinel) and np.all(host[guard + count :] == sentinel)
        assert_identical(results(ta), results(tb))


# ---- 12. the C++ program ----
def test_cpp_grid_histogram_on_gpu():
    from test_grid_histogram import build_cpp

    out = subprocess.run([build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
