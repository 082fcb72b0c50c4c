"""Wall time of propagate_grid() with observables next to what the same commit does without them: the whole
state into a device buffer (propagate_grid_device()) followed by cfunc.eval_device() over every row of it. Nothing here is
a threshold: the log (profiles/grid_observables_rates.log) is what DESIGN and the README quote.

  python profiles/grid_observables_rates.py              # on a GPU: measures, prints one line per figure
  python profiles/grid_observables_rates.py --rehearse   # without one: builds everything, prints the modules chosen

Workload: N outer Solar Systems, N_GRID grid points over T_END years, high_accuracy. Observables: the energy (36 of 36
state rows read) in one leg, the squared distance of bodies 1 and 2 (6 rows) in another. One warm-up call (code objects
loaded, buffers allocated), then REPS timed calls from the same initial state: the median with the smallest and the
largest. The wall time runs from the call to the synchronise behind it. The sizes of the output buffers follow from the
shapes: n_grid * n_obs * N * 8 bytes against n_grid * 36 * N * 8.

The post-step kernel alone: a kernel trace of one leg and one variant, so that every hy_grid_post in the trace is the same
kernel (the plain module and the modules with a section all call theirs hy_grid_post),

  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/grid_observables_rates.py --leg energy --only fused
  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/grid_observables_rates.py --leg energy --only full

and the same with --leg distance; the log quotes the hy_grid_post lines of the kernel statistics."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

N = 1 << 18
N_GRID = 65
T_END = 1000.0
REPS = 3


def legs():
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    vs = {repr(e): e for e in hy._to_sys(sys_).vars}
    d = [vs[a + "_1"] - vs[a + "_2"] for a in "xyz"]
    return sys_, [("energy", [hy.model.nbody_energy(6, masses=M, Gconst=G)]),
                  ("pair distance", [d[0] * d[0] + d[1] * d[1] + d[2] * d[2]])]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearse", action="store_true", help="build everything and print the choices, measure nothing")
    ap.add_argument("-n", type=int, default=N)
    ap.add_argument("--leg", choices=["energy", "distance"], help="one observable only")
    ap.add_argument("--only", choices=["fused", "full"], help="one variant only (for a kernel trace), no check")
    args = ap.parse_args()
    if not args.rehearse and hy.device_count() == 0:
        raise SystemExit("grid_observables_rates.py: no HIP device visible (use --rehearse without one)")
    n = args.n
    print("library build id %s" % hy.build_id())
    sys_, obs_legs = legs()
    if args.leg:
        obs_legs = [l for l in obs_legs if l[0].endswith(args.leg)]
    svars = hy._to_sys(sys_).vars
    st = configs.outer_ss_state(n, perturb=1e-6, seed=5)
    grid = np.linspace(0.0, T_END, N_GRID)
    ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)
    full_bytes = N_GRID * 36 * n * 8
    print("workload: %d outer Solar Systems, %d grid points over %g yr, stepper %s; full output %.1f MB"
          % (n, N_GRID, T_END, ta.hip_source_mode, full_bytes / 1e6))
    for name, obs in obs_legs:
        src, co = ta.grid_observables_module(obs)
        rows = src.split("hy_obs_rows[HY_NROWS] = {")[1].split("}")[0].count("u")
        mode = "staged" if "a.stage" in src else "registers"
        print("[module] %-13s %d observable(s) over %d of 36 state rows, samples held in %s, code object %d bytes"
              % (name, len(obs), rows, mode, len(co)))
    if args.rehearse:
        return
    import torch

    dev = torch.device("cuda:0")
    d_full = torch.empty((N_GRID, 36, n), dtype=torch.float64, device=dev)
    for name, obs in obs_legs:
        n_obs = len(obs)
        d_obs = torch.empty((N_GRID, n_obs, n), dtype=torch.float64, device=dev)
        cf = hy.cfunc(obs, vars=svars)

        def baseline():
            ta.propagate_grid_device(grid, d_full.data_ptr())
            for g in range(N_GRID):
                cf.eval_device(d_obs.data_ptr() + g * n_obs * n * 8, d_full.data_ptr() + g * 36 * n * 8, n)
            torch.cuda.synchronize()

        def grid_only():
            ta.propagate_grid_device(grid, d_full.data_ptr())

        def fused():
            ta.propagate_grid_device(grid, d_obs.data_ptr(), observables=obs)

        for what, fn, byts in (("full grid + cfunc pass", baseline, full_bytes + N_GRID * n_obs * n * 8),
                               ("full grid alone", grid_only, full_bytes),
                               ("observables in the grid loop", fused, N_GRID * n_obs * n * 8)):
            if args.only and (fn is baseline or (fn is fused) != (args.only == "fused")):
                continue
            t = timed(ta, st, fn)
            steps = sum(r[3] for r in ta.propagate_res)
            print("[wall] %-13s %-30s %.3f s median of %d calls (min %.3f, max %.3f), output buffers %.1f MB, %.4g system-steps/s"
                  % (name, what, t[len(t) // 2], len(t), t[0], t[-1], byts / 1e6, steps / t[len(t) // 2]))
            sys.stdout.flush()
        if args.only:
            continue
        # The two ways give the same bits.
        ref = d_obs.clone()
        ta.state = st
        ta.set_time(0.0)
        baseline()
        print("[check] %-13s fused == full grid + cfunc, bit for bit: %s" % (name, bool(torch.equal(ref.view(torch.int64), d_obs.view(torch.int64)))))


if __name__ == "__main__":
    main()
