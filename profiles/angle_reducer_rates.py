"""Rates of callback::angle_reducer on one MI355X, protocol of profiles/r06_model_rates.log: 262 144 systems,
propagate_until() over about 100 steps, every case timed after one untimed warm-up on the same card in the same process:
(a) no callback, (b) the library's angle_reducer (fused into the propagate kernel), (c) a Python callback doing the same
through ``ta.state``. model::pendulum with rotating initial conditions, then the chain of 16 pendula
(mixed_models.sine_lattice). Writes system-steps/s, the ratios b/a and b/c and the one-off compilation time of the fused
variant to profiles/angle_reducer_rates.log (or the file given as first argument)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import mixed_models as mm  # noqa: E402

N = 262144
TWOPI = float.fromhex("0x1.921fb54442d18p+2")


class host_reducer:
    def __init__(self, idx):
        self.idx = idx

    def __call__(self, ta):
        st = ta.state
        st[self.idx] = st[self.idx] - TWOPI * np.floor(st[self.idx] / TWOPI)
        ta.state = st
        return True


def timed(sys_, st, t_end, callback):
    rate = None
    for rep in range(2):  # (the first one is the warm-up: module load, buffers, compilation of the variant)
        ta = hy.taylor_adaptive_batch(sys_, st, N)
        ta.state = st
        ta.step()  # the state lives on the device from here on
        ta.synchronize()
        t0 = time.perf_counter()
        ta.propagate_until(t_end, callback=callback() if callback else None)
        steps = ta.last_total_steps
        ta.synchronize()
        rate = steps / (time.perf_counter() - t0)
    return rate, steps / N, ta


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "angle_reducer_rates.log")
    rng = np.random.RandomState(1)
    cases = []
    pend = hy.model.pendulum()
    st = np.stack([rng.uniform(0.0, 2 * np.pi, N), 10.0 + rng.uniform(0.0, 0.2, N)])
    cases.append(("model::pendulum, rotating", pend, st, 10.0, [0], pend.vars[:1]))
    lat = mm.sine_lattice(hy, 16)
    st = mm.sine_lattice_state(16, N, seed=3)
    st[:16] += 40.0
    cases.append(("sine_lattice(16), angles + 40", lat, st, 12.0, list(range(16)), [v for v, _ in lat[:16]]))
    lines = ["# profiles/angle_reducer_rates.py: %d systems, one MI355X, propagate_until(), wall clock of the call after one "
             "untimed warm-up; %s" % (N, hy.version())]
    for name, sys_, st, t_end, idx, vars_ in cases:
        a, spl, ta = timed(sys_, st, t_end, None)
        b, _, tb = timed(sys_, st, t_end, lambda: hy.callback.angle_reducer(vars_))
        path_b, comp = tb.last_callback_path, tb.angle_reduce_compile_seconds
        c, _, tc = timed(sys_, st, t_end, lambda: host_reducer(idx))
        lines.append("%-32s steps/system %.1f | %s" % (name, spl, ta.hip_source_mode[:90]))
        lines.append("    (a) no callback                      %.3g system-steps/s" % a)
        lines.append("    (b) angle_reducer (callback path %d)  %.3g system-steps/s" % (path_b, b))
        lines.append("    (c) Python callback through ta.state %.3g system-steps/s (callback path %d)" % (c, tc.last_callback_path))
        lines.append("    b/a = %.3f   b/c = %.1f   one-off compilation of the fused variant: %.2f s" % (b / a, b / c, comp))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
