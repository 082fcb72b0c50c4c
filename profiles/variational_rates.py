"""Rates of the variational integrators and of the Taylor-map cloud kernel, next to the plain systems on the
same commit. Nothing here is a threshold: the log (profiles/variational_rates.log) is what the README quotes.

  python profiles/variational_rates.py              # on a GPU: measures, prints one line per figure
  python profiles/variational_rates.py --rehearse   # without one: builds everything, prints the generators chosen

System-steps/s: total steps of one device-resident propagate_until() over the wall time up to the synchronise behind
it. A warm-up propagation of the same integrator (code objects loaded, buffers allocated) also gives a first rate, from
which the final time of the timed windows is chosen so that each lasts about WINDOW_S seconds; REPS windows are taken and
the median is reported with the smallest and the largest. The generator is the stage logger's verdict. Cloud kernel: HIP
events around a batch of launches sized the same way from a warm-up batch, REPS batches; operations and bytes are counted
from the shapes - per sample n_orig * (n_terms - 1) fma (2 flop) + (n_terms - 1 - n_args) products, and
(n_args + n_orig) * 8 bytes - and compared with the FP64 vector peak and the HBM peak of bench.py."""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

WINDOW_S = 0.6
REPS = 3
FP64_PEAK_TFLOPS = 78.6
HBM_PEAK_GBS = 8000.0

_log = []


def _capture_log():
    hy.set_logger_level("info")
    hy.set_log_callback(lambda level, msg: _log.append(msg))


def _generator_of(build):
    del _log[:]
    ta = build()
    lines = [m for m in _log if "generator" in m or "planner" in m or "stepper" in m]
    return ta, (lines[-1] if lines else ta.hip_source_mode)


def kepler_planar():
    x, y, vx, vy = hy.make_vars("x", "y", "vx", "vy")
    r3 = hy.pow(x * x + y * y, -1.5)
    return [(x, vx), (y, vy), (vx, -x * r3), (vy, -y * r3)]


def kepler_state(n, seed=1):
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.0, 0.3, n)
    return np.array([1.0 - e, np.zeros(n), np.zeros(n), np.sqrt((1.0 + e) / (1.0 - e))])


def pendulum_state(n, seed=2):
    rng = np.random.default_rng(seed)
    return np.array([rng.uniform(-2.0, 2.0, n), rng.uniform(-0.5, 0.5, n)])


def _one_window(ta, state, t_end):
    ta.state = state
    ta.set_time(0.0)
    ta.synchronize()
    t0 = time.perf_counter()
    ta.propagate_until(t_end)
    ta.synchronize()
    dt = time.perf_counter() - t0
    return sum(r[3] for r in ta.propagate_res), dt


def steps_per_second(ta, state, t_warm):
    """[(rate, steps, seconds)] of REPS windows of about WINDOW_S seconds each, and the final time they ran to."""
    _one_window(ta, state, t_warm)
    steps, dt = _one_window(ta, state, t_warm)
    # (The number of steps grows with the final time: scale it to the window. Twice, since the first estimate comes from a
    # window which may be much too short.)
    t_end = t_warm
    for _ in range(2):
        if dt < 0.8 * WINDOW_S:
            t_end *= WINDOW_S / max(dt, 1e-4)
            steps, dt = _one_window(ta, state, t_end)
    out = []
    for _ in range(REPS):
        steps, dt = _one_window(ta, state, t_end)
        out.append((steps / dt, steps, dt))
    return out, t_end


def stepper_legs(rehearse):
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    oss = hy.model.nbody(6, masses=M, Gconst=G)
    oss_vars = hy._to_sys(oss).vars
    legs = [
        ("pendulum", hy.model.pendulum(gconst=9.8), lambda s: hy.var_ode_sys(s, hy.var_args.vars, 1), pendulum_state, 1 << 18, (1000.0, 200.0), {}),
        ("planar Kepler", kepler_planar(), lambda s: hy.var_ode_sys(s, hy.var_args.vars, 1), kepler_state, 1 << 16, (1000.0, 200.0), {}),
        # Jupiter's six initial conditions (body 1 of the outer Solar System: rows 6 ... 11).
        ("outer Solar System wrt one body", oss, lambda s: hy.var_ode_sys(s, oss_vars[6:12], 1),
         lambda n: configs.outer_ss_state(n, perturb=1e-8, seed=11), 1 << 14, (2000.0, 5.0), {"high_accuracy": True}),
    ]
    for name, sys_, mk, st_fn, n, t_ends, kw in legs:
        st = st_fn(n)
        # (The final times here are those of the warm-up; steps_per_second() lengthens them to windows of WINDOW_S.)
        for what, s, t_end in (("plain", sys_, t_ends[0]), ("variational", mk(sys_), t_ends[1])):
            t0 = time.perf_counter()
            ta, gen = _generator_of(lambda: hy.taylor_adaptive_batch(s, st, n, **kw))
            build_s = time.perf_counter() - t0
            head = "[steps] %-32s %-11s dim %3d, N %7d, built in %5.1f s, generator: %s" % (name, what, ta.dim, n, build_s, gen)
            if rehearse:
                print(head)
                continue
            wins, t_used = steps_per_second(ta, ta.state.copy(), t_end)
            rates = sorted(w[0] for w in wins)
            print("%s | %.4g system-steps/s median of %d windows (min %.4g, max %.4g; %s; final time %.4g)"
                  % (head, rates[len(rates) // 2], len(wins), rates[0], rates[-1],
                     ", ".join("%d steps in %.3f s" % (w[1], w[2]) for w in wins), t_used))
            sys.stdout.flush()


def oscillators3():
    v = hy.make_vars("x1", "x2", "x3", "v1", "v2", "v3")
    ks = (1.0, 1.7, 2.9)
    return [(v[i], v[3 + i]) for i in range(3)] + [(v[3 + i], -ks[i] * v[i]) for i in range(3)]


def cloud_legs(rehearse):
    import torch

    n_sys, ns, reps = 256, 1 << 16, 20
    for order in (2, 3):
        vs = hy.var_ode_sys(oscillators3(), hy.var_args.vars, order)
        n_terms = math.comb(6 + order, order)
        t0 = time.perf_counter()
        rng = np.random.default_rng(order)
        # (The state is what a propagation would leave: any finite coefficients do for a rate.)
        ta = hy.taylor_adaptive_batch(vs, rng.uniform(-1, 1, (6 * n_terms, n_sys)), emitter="table")
        note = hy.taylor_map_source(6, 6, order)[1]
        head = "[cloud] (6, 6, %d): %s; integrator built in %.1f s" % (order, note, time.perf_counter() - t0)
        if rehearse:
            print(head)
            continue
        print(head)
        dev = torch.device("cuda:0")
        flop = 6 * (n_terms - 1) * 2 + (n_terms - 1 - 6)
        for shared in (False, True):
            d_delta = torch.rand((6, ns) if shared else (n_sys, 6, ns), device=dev, dtype=torch.float64) * 0.02 - 0.01
            d_out = torch.empty((n_sys, 6, ns), device=dev, dtype=torch.float64)
            byts = (6 + 6) * 8 if not shared else 6 * 8  # (a shared cloud is read from the caches after its first use)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def batch(k):
                torch.cuda.synchronize()
                e0.record()
                for _ in range(k):
                    ta.eval_taylor_map_cloud(d_delta, d_out, ns, shared=shared)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / k

            # Warm-up batch, then batches of about WINDOW_S seconds.
            k = max(reps, int(WINDOW_S * 1e3 / batch(reps)))
            all_ms = sorted(batch(k) for _ in range(REPS))
            ms = all_ms[len(all_ms) // 2]
            samples = n_sys * ns
            tfl, gbs = samples * flop / ms / 1e9, samples * byts / ms / 1e6
            t_min = max(samples * flop / (FP64_PEAK_TFLOPS * 1e12), samples * byts / (HBM_PEAK_GBS * 1e9)) * 1e3
            bound = "fp64" if samples * flop / (FP64_PEAK_TFLOPS * 1e12) > samples * byts / (HBM_PEAK_GBS * 1e9) else "hbm"
            print("[cloud] (6, 6, %d) %-10s %d systems x %d samples: %.3f ms per launch (median of %d batches of %d launches, min %.3f, "
                  "max %.3f), %.4g samples/s, %.0f GB/s (%.2f of HBM "
                  "peak), %.2f TFLOP/s (%.2f of the FP64 vector peak); roofline %.3f ms (%s-bound): %.2f of it"
                  % (order, "shared" if shared else "per-system", n_sys, ns, ms, REPS, k, all_ms[0], all_ms[-1], samples / ms * 1e3, gbs, gbs / HBM_PEAK_GBS, tfl,
                     tfl / FP64_PEAK_TFLOPS, t_min, bound, t_min / ms))
            sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rehearse", action="store_true", help="build everything and print the choices, measure nothing")
    args = ap.parse_args()
    if not args.rehearse and hy.device_count() == 0:
        raise SystemExit("variational_rates.py: no HIP device visible (use --rehearse without one)")
    _capture_log()
    print("library build id %s" % hy.build_id())
    stepper_legs(args.rehearse)
    cloud_legs(args.rehearse)


if __name__ == "__main__":
    main()
