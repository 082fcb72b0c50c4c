"""Wall time of propagate_grid() with ensemble histograms next to what the commit before the feature can do: the
observables of every grid point into a full device buffer (propagate_grid_device(observables=...)) followed by
torch.bucketize(..., right=True) and a bincount per row. Nothing here is a threshold: the log
(profiles/grid_histogram_rates.log) is what DESIGN and the README quote.

  python profiles/grid_histogram_rates.py              # on a GPU: measures, prints one line per figure
  python profiles/grid_histogram_rates.py --rehearse   # without one: builds everything, prints the modules chosen

Workload: N outer Solar Systems over T_END years, high_accuracy, observables = the energy minus the median energy of the
ensemble at the start and the squared distance of bodies 1 and 2, 256 bins each over the range which a pre-pass finds - the
first 4 096 systems over 65 points, and the whole ensemble at the start -, widened by 5 %: two populated histograms;
grids of 65 and of 1 025 points. One warm-up call, then REPS
timed calls from the same initial state: the median with the smallest and the largest. HEYOKA_AMD_GRID_HIST (and
HEYOKA_AMD_GRID_HIST_TURNS) in the environment choose the way of merging. The last line per grid checks every counter of the
last fused call against numpy.searchsorted and numpy.bincount over the full buffer of the last baseline call.

The post-step kernel alone: a kernel trace of one grid and one variant, so that every hy_grid_post in the trace is the same
kernel,

  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_histogram_rates.py --points 257 --only hist --reps 1
  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_histogram_rates.py --points 257 --only full --reps 1
  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_histogram_rates.py --synthetic onebin --reps 1
  python profiles/grid_histogram_rates.py --kernels DIR LABEL     # the [kernel] line of such a trace

--synthetic onebin|uniform: N pendula whose observable is par[0], every system in one bin or the systems uniform over the 256
bins - the two extremes of contention, where the kernel does little else than merge."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

from grid_ensemble_rates import timed  # noqa: E402
from grid_statistics_rates import kernel_lines, observables  # noqa: E402

N = 1 << 18
POINTS = (65, 1025)
T_END = 1000.0
BINS = 256
PRE = 4096
STATS = ["count", "mean", "min", "max", "sum_sq"]


def how():
    mode = os.environ.get("HEYOKA_AMD_GRID_HIST") or "hybrid"
    return mode + (" K=%s" % (os.environ.get("HEYOKA_AMD_GRID_HIST_TURNS") or "1") if mode == "hybrid" else "")


def synthetic(args):
    """The merge alone: pendula, observable par[0]."""
    n = args.n
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -hy.par[1] * hy.sin(x))]
    rng = np.random.RandomState(3)
    p0 = np.full(n, 100.5) if args.synthetic == "onebin" else rng.uniform(0.0, BINS, n)
    pars = np.stack([p0, np.full(n, 9.8)])
    st = np.stack([rng.uniform(0.1, 1.0, n), rng.uniform(-0.5, 0.5, n)])
    ta = hy.taylor_adaptive_batch(sys_, st, n, pars=pars, high_accuracy=True)
    edges = [np.arange(BINS + 1.0)]
    grid = np.linspace(0.0, 20.0, args.points or 65)
    print("[synthetic] %s: %d pendula, observable par[0], %d bins, %d points, %s" % (args.synthetic, n, BINS, grid.size, how()))
    if args.rehearse:
        ta.grid_observables_module([hy.par[0]], ensemble_histograms=edges)
        return
    got = {}

    def fused():
        got["h"] = ta.propagate_grid(grid, observables=[hy.par[0]], ensemble_histograms=edges)[1]

    t = timed(ta, st, fused, args.reps)
    exp = np.bincount(np.searchsorted(edges[0], p0, side="right"), minlength=BINS + 2)
    ok = bool(np.all(got["h"].counts(0) == exp[None, :]))
    print("[wall] %-9s %-28s %.3f s median of %d calls (min %.3f, max %.3f); [check] every row equals the bincount of par[0]: %s"
          % (args.synthetic, how(), t[len(t) // 2], len(t), t[0], t[-1], ok))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearse", action="store_true", help="build everything and print the choices, measure nothing")
    ap.add_argument("-n", type=int, default=N)
    ap.add_argument("--points", type=int, help="one grid only")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["hist", "full", "both"], help="one variant only (for a kernel trace), no check")
    ap.add_argument("--synthetic", choices=["onebin", "uniform"], help="the merge alone, through par[0]")
    ap.add_argument("--kernels", nargs=2, metavar=("DIR", "LABEL"), help="summarise the kernel traces under DIR")
    args = ap.parse_args()
    if args.kernels:
        kernel_lines(*args.kernels)
        return
    if not args.rehearse and hy.device_count() == 0:
        raise SystemExit("grid_histogram_rates.py: no HIP device visible (use --rehearse without one)")
    print("library build id %s, HEYOKA_AMD_GRID_HIST: %s" % (hy.build_id(), how()))
    if args.synthetic:
        synthetic(args)
        return
    n = args.n
    sys_, obs = observables()
    n_obs = len(obs)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)
    print("workload: %d outer Solar Systems over %g yr, stepper %s"
          % (n, T_END, ta.hip_source_mode.split(":")[0].split(" [")[0] + (" v5" if "v5" in ta.hip_source_mode else "")))
    if args.rehearse:
        e0, edges = 0.0, [np.linspace(-1.0, 1.0, BINS + 1)] * 2
    else:
        # The edges are data, made as a user would make them: from a cheap pre-pass, the first PRE systems over a grid of 65
        # points, together with the whole ensemble at the start; the range of each observable widened by 5 %.
        y0 = ta.propagate_grid(np.array([0.0]), observables=obs)[1][0]
        e0 = float(np.median(y0[0]))
        tp = hy.taylor_adaptive_batch(sys_, st[:, :PRE].copy(), PRE, high_accuracy=True)
        yp = tp.propagate_grid(np.linspace(0.0, T_END, 65), observables=obs)[1]
        rng = [np.concatenate([y0[o], yp[:, o, :].reshape(-1)]) - (e0 if o == 0 else 0.0) for o in range(n_obs)]
        edges = [np.linspace(r.min() - 0.05 * np.ptp(r), r.max() + 0.05 * np.ptp(r), BINS + 1) for r in rng]
        ta.state = st
        ta.set_time(0.0)
    obs = [obs[0] - e0, obs[1]]
    for what, kw in (("observables", {}), ("histograms", dict(ensemble_histograms=edges)),
                     ("both", dict(ensemble_histograms=edges, ensemble_statistics=STATS))):
        src, co = ta.grid_observables_module(obs, **kw)
        print("[module] %-11s %d observables, samples held in %s%s, code object %d bytes"
              % (what, n_obs, "the staging buffer" if "a.stage" in src else "registers",
                 ", %s words per grid point, %s" % (src.split("#define HY_HIST_W ")[1].split("u")[0], how()) if kw else "", len(co)))
    if args.rehearse:
        return
    import torch

    dev = torch.device("cuda:0")
    t_edges = [torch.tensor(e, dtype=torch.float64, device=dev) for e in edges]
    for n_grid in ([args.points] if args.points else POINTS):
        grid = np.linspace(0.0, T_END, n_grid)
        d_full = torch.empty((n_grid, n_obs, n), dtype=torch.float64, device=dev) if args.only in (None, "full") else None
        red, got = {}, {}
        rows = torch.arange(n_grid, device=dev)[:, None] * (BINS + 3) if d_full is not None else None

        def full_only():
            ta.propagate_grid_device(grid, d_full.data_ptr(), observables=obs)

        def baseline():
            full_only()
            for o in range(n_obs):
                v = d_full[:, o, :]
                idx = torch.bucketize(v, t_edges[o], right=True)
                idx = torch.where(torch.isnan(v), BINS + 2, idx)  # (a slot of their own, dropped below)
                red[o] = torch.bincount((idx + rows).view(-1), minlength=n_grid * (BINS + 3)).view(n_grid, BINS + 3)[:, : BINS + 2]
            torch.cuda.synchronize()

        def fused():
            got["h"] = ta.propagate_grid(grid, observables=obs, ensemble_histograms=edges)[1]

        def fused_device():
            ta.propagate_grid_device(grid, d_acc.data_ptr(), observables=obs, ensemble_histograms=edges)

        def fused_both():
            got["both"] = ta.propagate_grid(grid, observables=obs, ensemble_histograms=edges, ensemble_statistics=STATS)[1]

        hist_words = hy.ensemble_histogram_accumulators(n_grid, edges).raw.size
        ens_words = hy.ensemble_accumulators(n_grid, n_obs, STATS).raw.size
        d_acc = torch.empty(hist_words, dtype=torch.int64, device=dev)
        full_bytes = n_grid * n_obs * n * 8
        label = "%d points" % n_grid
        for what, fn in (("observables + torch.bucketize + bincount per row", baseline), ("observables alone", full_only),
                         ("histograms in the grid loop (%s)" % how(), fused),
                         ("the same, words into a device buffer (%s)" % how(), fused_device),
                         ("histograms and %s (%s)" % (", ".join(STATS), how()), fused_both)):
            if args.only and fn is not {"hist": fused, "full": full_only, "both": fused_both}[args.only]:
                continue
            t = timed(ta, st, fn, args.reps)
            steps = sum(r[3] for r in ta.propagate_res)
            if fn in (baseline, full_only):
                byts = full_bytes + (full_bytes + hist_words * 8 if fn is baseline else 0)  # (the indices are as large as a column)
            else:
                byts = (2 * (hist_words + (ens_words if fn is fused_both else 0)) + edges[0].size * 2 + (hist_words if fn is fused_device else 0)) * 8
            print("[wall] %-11s %-62s %.3f s median of %d calls (min %.3f, max %.3f), output buffers %.1f MB, %.4g system-steps/s"
                  % (label, what, t[len(t) // 2], len(t), t[0], t[-1], byts / 1e6, steps / t[len(t) // 2]))
            sys.stdout.flush()
        if args.only:
            continue
        # The last fused calls and the last baseline() started from the same state.
        t0 = time.perf_counter()
        ok = {"histograms alone": True, "with the ensemble statistics": True, "torch baseline": True}
        acc, hboth = got["both"]
        total = 0
        for g in range(n_grid):
            full_g = d_full[g].cpu().numpy()
            for o in range(n_obs):
                v = full_g[o]
                exp = np.bincount(np.searchsorted(edges[o], v[~np.isnan(v)], side="right"), minlength=BINS + 2)
                total += int(exp.sum())
                ok["histograms alone"] &= bool(np.array_equal(got["h"].counts(o)[g], exp))
                ok["with the ensemble statistics"] &= bool(np.array_equal(hboth.counts(o)[g], exp))
        for o in range(n_obs):
            ok["torch baseline"] &= bool(np.array_equal(red[o].cpu().numpy(), got["h"].counts(o).astype(np.int64)))
        count_ok = bool(np.array_equal(acc.values[:, :, 0], np.stack([hboth.counts(o).sum(axis=1) for o in range(n_obs)], axis=1).astype(float)))
        open_slots = [int(got["h"].counts(o)[:, 0].sum() + got["h"].counts(o)[:, -1].sum()) for o in range(n_obs)]
        print("[check] %-11s every counter against numpy.searchsorted + bincount of the full buffer (%d x %d x %d values, %d counted, "
              "%s in the open slots, %.0f s): %s; the counters of a record sum to the count statistic: %s; all: %s"
              % (label, n_grid, n_obs, n, total, open_slots, time.perf_counter() - t0,
                 ", ".join("%s %s" % kv for kv in ok.items()), count_ok, all(ok.values()) and count_ok))
        del d_full, red


if __name__ == "__main__":
    main()
