"""Wall time of propagate_grid_device() with statistics next to what the commit before the feature can do: the
observables of every grid point into a full device buffer (propagate_grid_device(observables=...)) followed by torch.amin /
amax / argmax over the point axis. Nothing here is a threshold: the log (profiles/grid_statistics_rates.log) is what DESIGN
and the README quote.

  python profiles/grid_statistics_rates.py              # on a GPU: measures, prints one line per figure
  python profiles/grid_statistics_rates.py --rehearse   # without one: builds everything, prints the modules chosen

Workload: N outer Solar Systems over T_END years, high_accuracy, observables = the energy and the squared distance of bodies
1 and 2, statistics min, max, t_max; grids of 65 and of 1 025 points. One warm-up call (code objects loaded, buffers
allocated), then REPS timed calls from the same initial state: the median with the smallest and the largest. The wall time
runs from the call to the synchronise behind it. The output buffers follow from the shapes: n_grid * n_obs * N * 8 bytes plus
the results of the reduction against 2 * n_obs * n_stat * N * 8 bytes of accumulators and shadow copy.

The post-step kernel alone: a kernel trace of one grid and one variant, so that every hy_grid_post in the trace is the same
kernel,

  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_statistics_rates.py --points 1025 --only folded
  rocprofv3 --kernel-trace -d DIR --output-format csv -- python profiles/grid_statistics_rates.py --points 1025 --only full
  python profiles/grid_statistics_rates.py --kernels DIR LABEL     # the [kernel] line of such a trace"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

N = 1 << 18
POINTS = (65, 1025)
T_END = 1000.0
REPS = 3
STATS = ["min", "max", "t_max"]


def observables():
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    vs = {repr(e): e for e in hy._to_sys(sys_).vars}
    d = [vs[a + "_1"] - vs[a + "_2"] for a in "xyz"]
    return sys_, [hy.model.nbody_energy(6, masses=M, Gconst=G), d[0] * d[0] + d[1] * d[1] + d[2] * d[2]]


def timed(ta, st, fn):
    out = []
    for k in range(REPS + 1):
        ta.state = st
        ta.set_time(0.0)
        ta.synchronize()
        t0 = time.perf_counter()
        fn()
        ta.synchronize()
        if k != 0:  # (the first call is the warm-up)
            out.append(time.perf_counter() - t0)
    return sorted(out)


def kernel_lines(directory, label):
    """The durations of hy_grid_post / hy_grid_obs0 in the kernel traces (csv) under ``directory``."""
    dur = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0]
                if name in ("hy_grid_post", "hy_grid_obs0", "hy_grid_unsample"):
                    dur.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    for name in sorted(dur):
        d = sorted(dur[name])
        print("[kernel] %-22s %-13s %d launches, median %.4f ms (min %.4f, max %.4f), total %.3f ms"
              % (label, name, len(d), d[len(d) // 2], d[0], d[-1], sum(d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearse", action="store_true", help="build everything and print the choices, measure nothing")
    ap.add_argument("-n", type=int, default=N)
    ap.add_argument("--points", type=int, help="one grid only")
    ap.add_argument("--only", choices=["folded", "full"], help="one variant only (for a kernel trace), no check")
    ap.add_argument("--kernels", nargs=2, metavar=("DIR", "LABEL"), help="summarise the kernel traces under DIR")
    args = ap.parse_args()
    if args.kernels:
        kernel_lines(*args.kernels)
        return
    if not args.rehearse and hy.device_count() == 0:
        raise SystemExit("grid_statistics_rates.py: no HIP device visible (use --rehearse without one)")
    n = args.n
    print("library build id %s" % hy.build_id())
    sys_, obs = observables()
    n_obs, n_stat = len(obs), len(STATS)
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)
    print("workload: %d outer Solar Systems over %g yr, stepper %s" % (n, T_END, ta.hip_source_mode.split(":")[0].split(" [")[0] + (" v5" if "v5" in ta.hip_source_mode else "")))
    for what, kw in (("observables", {}), ("statistics", dict(statistics=STATS))):
        src, co = ta.grid_observables_module(obs, **kw)
        print("[module] %-11s %d observables, samples held in %s%s, code object %d bytes"
              % (what, n_obs, "the staging buffer" if "a.stage" in src else "registers",
                 ", %s accumulators per system" % src.split("#define HY_NSLOT ")[1].split("u")[0] if kw else "", len(co)))
    if args.rehearse:
        return
    import torch

    dev = torch.device("cuda:0")
    for n_grid in ([args.points] if args.points else POINTS):
        grid = np.linspace(0.0, T_END, n_grid)
        d_full = torch.empty((n_grid, n_obs, n), dtype=torch.float64, device=dev) if args.only != "folded" else None
        d_st = torch.empty((n_obs, n_stat, n), dtype=torch.float64, device=dev)
        red = {}

        def full_only():
            ta.propagate_grid_device(grid, d_full.data_ptr(), observables=obs)

        def baseline():
            full_only()
            red["min"], red["max"] = torch.amin(d_full, dim=0), torch.amax(d_full, dim=0)
            red["argmax"] = torch.argmax(d_full, dim=0)
            torch.cuda.synchronize()

        def folded():
            ta.propagate_grid_device(grid, d_st.data_ptr(), observables=obs, statistics=STATS)

        full_bytes, red_bytes = n_grid * n_obs * n * 8, 3 * n_obs * n * 8
        ta_slots = 2 * n_obs * n_stat * n * 8
        label = "%d points" % n_grid
        for what, fn, byts in (("observables + torch reduction", baseline, full_bytes + red_bytes),
                               ("observables alone", full_only, full_bytes),
                               ("statistics in the grid loop", folded, ta_slots + n_obs * n_stat * n * 8)):
            if args.only and (fn is baseline or (fn is folded) != (args.only == "folded")):
                continue
            t = timed(ta, st, fn)
            steps = sum(r[3] for r in ta.propagate_res)
            print("[wall] %-11s %-30s %.3f s median of %d calls (min %.3f, max %.3f), output buffers %.1f MB (grid itself %.1f MB), "
                  "%.4g system-steps/s" % (label, what, t[len(t) // 2], len(t), t[0], t[-1], byts / 1e6, n_grid * n * 8 / 1e6,
                                           steps / t[len(t) // 2]))
            sys.stdout.flush()
        if args.only:
            continue
        # The last folded() and the last baseline() started from the same state: min and max, bit for bit. (No NaN here.)
        eq = lambda a, b: bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))  # noqa: E731
        # (t_max is the FIRST grid time of the maximum; torch.argmax names any of several equal maxima: the values at the two.)
        at = torch.gather(d_full, 0, torch.searchsorted(torch.as_tensor(grid, device=dev), d_st[:, 2].contiguous())[None])[0]
        print("[check] %-11s min == torch.amin: %s, max == torch.amax: %s, observable at t_max == max: %s, bit for bit"
              % (label, eq(d_st[:, 0], red["min"]), eq(d_st[:, 1], red["max"]), eq(at, red["max"])))
        del d_full, red


if __name__ == "__main__":
    main()
