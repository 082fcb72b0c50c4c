"""Rates of step_action on one MI355X, protocol of profiles/angle_reducer_rates.py: 262 144 systems, one
propagate_until() over about 100 steps (pendulum) / 55 steps (outer Solar System), timed three times (median, min and max reported) after an untimed warm-up - a short
propagation with the same callback: module load, buffers, compilation of the action's kernel - on the same card in the same
process: (a) no callback, (b) the action, (c) the same action as a Python host callback (values from hy.cfunc on host
arrays, the mask ``ta.last_h != 0``, written through ``ta.state``). model::pendulum with rotating initial conditions and
v <- (1 - 1e-6) v, then the outer Solar System with the velocity of one body scaled by 1 + 1e-12. A fourth run of (b) with
the event timing on reads the duration of the hy_step_action launches from HIP events. Writes system-steps/s to
profiles/step_action_rates.log (or the file given as first argument)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

N = 262144


class host_action:
    def __init__(self, svars, assignments):
        names = [repr(s) for s in svars]
        self.rows = [names.index(repr(lhs)) for lhs, _ in assignments]
        self.cf = hy.cfunc([rhs for _, rhs in assignments], vars=svars)

    def __call__(self, ta):
        st = ta.state
        mask = ta.last_h != 0
        out = self.cf(st)
        for k, row in enumerate(self.rows):
            st[row, mask] = out[k, mask]
        ta.state = st
        return True


def timed(sys_, st, t_warm, t_end, callback, timing=False, **kw):
    rates, steps, ta = [], 0, None
    for rep in range(4):  # (the first one is the warm-up)
        ta = hy.taylor_adaptive_batch(sys_, st, N, **kw)
        ta.state = st
        ta.step()  # the state lives on the device from here on
        if timing:
            ta.set_event_timing(True)
        ta.synchronize()
        t0 = time.perf_counter()
        ta.propagate_until(t_warm if rep == 0 else t_end, callback=callback() if callback else None)
        steps = ta.last_total_steps
        ta.synchronize()
        if rep != 0:
            rates.append(steps / (time.perf_counter() - t0))
        if timing and rep == 1:
            break
    return sorted(rates), steps / N, ta


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_action_rates.log")
    rng = np.random.RandomState(1)
    cases = []
    pend = hy.model.pendulum()
    pv = pend.vars
    st = np.stack([rng.uniform(0.0, 2 * np.pi, N), 10.0 + rng.uniform(0.0, 0.2, N)])
    cases.append(("model::pendulum, rotating", pend, st, 0.5, 10.0, pv, [(pv[1], (1 - 1e-6) * pv[1])], {}))
    oss = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
    ov = hy._to_sys(oss).vars
    asg = [(ov[9 + k], (1.0 + 1e-12) * ov[9 + k]) for k in range(3)]
    cases.append(("outer Solar System", oss, configs.outer_ss_state(N, perturb=1e-3, seed=3), 2.0, 40.0, ov, asg,
                  dict(high_accuracy=True)))
    lines = ["# profiles/step_action_rates.py: %d systems, one MI355X, propagate_until(), wall clock of the call, median [min, max] "
             "of three after an untimed warm-up; %s" % (N, hy.version())]

    def fmt(r):
        return "%.3g [%.3g, %.3g] system-steps/s" % (r[len(r) // 2], r[0], r[-1])

    for name, sys_, st, t_warm, t_end, svars, asg, kw in cases:
        a, spl, ta = timed(sys_, st, t_warm, t_end, None, **kw)
        b, _, tb = timed(sys_, st, t_warm, t_end, lambda: hy.step_action(asg), **kw)
        path_b = tb.last_callback_path
        _, _, tt = timed(sys_, st, t_warm, t_end, lambda: hy.step_action(asg), timing=True, **kw)
        ms, launches = tt.step_action_kernel_ms
        c, _, tc = timed(sys_, st, t_warm, t_end, lambda: host_action(svars, asg), **kw)
        lines.append("%-28s steps/system %.1f | %s" % (name, spl, ta.hip_source_mode[:90]))
        lines.append("    (a) no callback                      " + fmt(a))
        lines.append("    (b) step_action (callback path %d)    " % path_b + fmt(b))
        lines.append("    (c) Python callback through ta.state " + fmt(c) + " (callback path %d)" % tc.last_callback_path)
        mid = [r[len(r) // 2] for r in (a, b, c)]
        lines.append("    b/a = %.3f   b/c = %.1f   hy_step_action: %.4f ms per launch (HIP events, %d launches)"
                     % (mid[1] / mid[0], mid[1] / mid[2], ms / max(launches, 1), launches))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
