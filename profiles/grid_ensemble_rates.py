"""Wall time of propagate_grid() with ensemble statistics next to what the commit before the feature can do: the
observables of every grid point into a full device buffer (propagate_grid_device(observables=...)) followed by torch.nansum
(of the values and of their squares), amin, amax and a count over the lane axis. Nothing here is a threshold: the log
(profiles/grid_ensemble_rates.log) is what DESIGN and the README quote.

  python profiles/grid_ensemble_rates.py              # on a GPU: measures, prints one line per figure
  python profiles/grid_ensemble_rates.py --rehearse   # without one: builds everything, prints the modules chosen

Workload: N outer Solar Systems over T_END years, high_accuracy, observables = the energy and the squared distance of bodies
1 and 2, ensemble statistics count, mean, min, max, sum_sq; grids of 65 and of 1 025 points. One warm-up call, then REPS timed
calls from the same initial state: the median with the smallest and the largest. HEYOKA_AMD_GRID_ENS=peratomic in the
environment measures the module without the aggregation per wavefront (--reps 1 keeps that short). The last line per grid
checks the values of the last fused call against a fold of the full buffer of the last baseline call which shares no code
with the library: integer mantissas summed per exponent in numpy, the total as one Python integer, one rounding by Fraction.

The post-step kernel alone: a kernel trace of one grid and one variant, so that every hy_grid_post in the trace is the same
kernel,

  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_ensemble_rates.py --points 1025 --only ensemble
  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_ensemble_rates.py --points 1025 --only full
  python profiles/grid_ensemble_rates.py --kernels DIR LABEL     # the [kernel] line of such a trace"""
import argparse
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

from grid_statistics_rates import kernel_lines, observables  # noqa: E402

N = 1 << 18
POINTS = (65, 1025)
T_END = 1000.0
STATS = ["count", "mean", "min", "max", "sum_sq"]


def timed(ta, st, fn, reps):
    out = []
    for k in range(reps + 1):
        ta.state = st
        ta.set_time(0.0)
        ta.synchronize()
        t0 = time.perf_counter()
        fn()
        ta.synchronize()
        if k != 0:  # (the first call is the warm-up)
            out.append(time.perf_counter() - t0)
    return sorted(out)


def exact_sum(v):
    """The exact sum of the finite doubles v, rounded once: mantissas as integers, summed in two 32-bit halves per exponent."""
    m, e = np.frexp(v)
    mi = np.ldexp(m, 53).astype(np.int64)
    e = e.astype(np.int64) - 53
    lo, hi = mi & 0xFFFFFFFF, mi >> 32  # (hi keeps the sign: mi == (hi << 32) + lo)
    e0, total = int(e.min()), 0
    for ev in range(e0, int(e.max()) + 1):
        k = e == ev
        if k.any():
            total += ((int(hi[k].sum()) << 32) + int(lo[k].sum())) << (ev - e0)
    s = Fraction(total) * Fraction(2) ** e0
    return float(s) if s != 0 else 0.0


def reference(row):
    """count, mean, min, max, sum_sq of one row of the full buffer (one observable, all lanes): NaN skipped, all finite."""
    v = row[~np.isnan(row)]
    assert v.size and np.isfinite(v).all()
    return [float(v.size), float(np.float64(exact_sum(v)) / np.float64(v.size)), v.min(), v.max(), exact_sum(v * v)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearse", action="store_true", help="build everything and print the choices, measure nothing")
    ap.add_argument("-n", type=int, default=N)
    ap.add_argument("--points", type=int, help="one grid only")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["ensemble", "full"], help="one variant only (for a kernel trace), no check")
    ap.add_argument("--kernels", nargs=2, metavar=("DIR", "LABEL"), help="summarise the kernel traces under DIR")
    args = ap.parse_args()
    if args.kernels:
        kernel_lines(*args.kernels)
        return
    if not args.rehearse and hy.device_count() == 0:
        raise SystemExit("grid_ensemble_rates.py: no HIP device visible (use --rehearse without one)")
    n = args.n
    how = os.environ.get("HEYOKA_AMD_GRID_ENS") or "aggregate"
    print("library build id %s, HEYOKA_AMD_GRID_ENS=%s" % (hy.build_id(), how))
    sys_, obs = observables()
    n_obs, n_stat = len(obs), len(STATS)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)
    print("workload: %d outer Solar Systems over %g yr, stepper %s" % (n, T_END, ta.hip_source_mode.split(":")[0].split(" [")[0] + (" v5" if "v5" in ta.hip_source_mode else "")))
    for what, kw in (("observables", {}), ("ensemble", dict(ensemble_statistics=STATS))):
        src, co = ta.grid_observables_module(obs, **kw)
        print("[module] %-11s %d observables, samples held in %s%s, code object %d bytes"
              % (what, n_obs, "the staging buffer" if "a.stage" in src else "registers",
                 ", %s words per grid point and observable, %s" % (src.split("#define HY_ENS_WORDS ")[1].split("u")[0], how) if kw else "",
                 len(co)))
    if args.rehearse:
        return
    import torch

    dev = torch.device("cuda:0")
    for n_grid in ([args.points] if args.points else POINTS):
        grid = np.linspace(0.0, T_END, n_grid)
        d_full = torch.empty((n_grid, n_obs, n), dtype=torch.float64, device=dev) if args.only != "ensemble" else None
        red, got = {}, {}

        def full_only():
            ta.propagate_grid_device(grid, d_full.data_ptr(), observables=obs)

        def baseline():
            full_only()
            red["sum"], red["sum_sq"] = torch.nansum(d_full, dim=2), torch.nansum(d_full * d_full, dim=2)
            red["min"], red["max"] = torch.amin(d_full, dim=2), torch.amax(d_full, dim=2)
            red["count"] = (~torch.isnan(d_full)).sum(dim=2)
            torch.cuda.synchronize()

        def fused():
            got["acc"] = ta.propagate_grid(grid, observables=obs, ensemble_statistics=STATS)[1]

        def fused_device():
            ta.propagate_grid_device(grid, d_acc.data_ptr(), observables=obs, ensemble_statistics=STATS)

        d_acc = torch.empty(hy.ensemble_accumulators(n_grid, n_obs, STATS).raw.size, dtype=torch.int64, device=dev)
        full_bytes, red_bytes = n_grid * n_obs * n * 8, 5 * n_grid * n_obs * 8
        label = "%d points" % n_grid
        for what, fn in (("observables + torch reduction", baseline), ("observables alone", full_only),
                         ("ensemble statistics in the grid loop (%s)" % how, fused),
                         ("the same, words into a device buffer (%s)" % how, fused_device)):
            if args.only and (fn is baseline or fn is fused_device or (fn is fused) != (args.only == "ensemble")):
                continue
            t = timed(ta, st, fn, args.reps)
            steps = sum(r[3] for r in ta.propagate_res)
            byts = 2 * d_acc.numel() * 8 + (d_acc.numel() * 8 if fn is fused_device else 0) if fn in (fused, fused_device) else full_bytes + (red_bytes + full_bytes if fn is baseline else 0)
            print("[wall] %-11s %-52s %.3f s median of %d calls (min %.3f, max %.3f), output buffers %.1f MB, %.4g system-steps/s"
                  % (label, what, t[len(t) // 2], len(t), t[0], t[-1], byts / 1e6, steps / t[len(t) // 2]))
            sys.stdout.flush()
        if args.only:
            continue
        # The last fused() and the last baseline() started from the same state.
        t0 = time.perf_counter()
        val = got["acc"].values
        exp = np.empty_like(val)
        for g in range(n_grid):
            rows = d_full[g].cpu().numpy()
            for o in range(n_obs):
                exp[g, o] = reference(rows[o])
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)  # noqa: E731
        ok = [bool(np.array_equal(bits(val[:, :, k]), bits(exp[:, :, k]))) for k in range(n_stat)]
        # (What the order-dependent float64 reduction of the baseline gives: how many of its sums are the exact ones.)
        ts = red["sum"].cpu().numpy()
        mean_b = ts / red["count"].cpu().numpy()
        print("[baseline] %-8s torch.nansum / count equals the correctly rounded mean in %d of %d cells (largest difference %.3g relative)"
              % (label, int((mean_b == exp[:, :, 1]).sum()), mean_b.size, float(np.max(np.abs(mean_b - exp[:, :, 1]) / np.abs(exp[:, :, 1])))))
        print("[check] %-11s %s against the fold of the full buffer in integer arithmetic (%d x %d x %d values, %.0f s), bit for bit: %s"
              % (label, ", ".join("%s %s" % (s, k) for s, k in zip(STATS, ok)), n_grid, n_obs, n, time.perf_counter() - t0, all(ok)))
        del d_full, red


if __name__ == "__main__":
    main()
