"""Cost of a terminal-event action (hy.event_action) per lock-step step(), on one MI355X.

Two workloads, 1 048 576 systems each:
  oscillators  x' = v, v' = -x with phases spread over the circle, terminal event x = 0 (downwards), v <- -0.8 v;
  outer_ss     the events workload of bench.py (outer Solar Systems spread over 30 yr of their orbits, Jupiter and Saturn
               crossing y = 0 as non-terminal events with counters) plus Uranus crossing y = 0 as a terminal event whose
               callback scales Uranus' velocity by 1 + 1e-9.
Four figures per workload, the variants interleaved round by round in one process:
  (a) the action, applied on the device;
  (b) the same events with counting callbacks - the floor: that path does no per-event host work either;
  (c) the same action as a Python callback (host loop);
  (d) the action's kernel alone, from HIP events around its launches (event timing on, further steps of (a)).
Usage: python profiles/event_action_rates.py [--n 1048576] [--rounds 3] [--steps 6] [--out profiles/event_action_rates.log]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

BOUNCE, KICK = -0.8, 1.0 + 1e-9


def oscillators(n):
    x, v = hy.make_vars("x", "v")
    rng = np.random.RandomState(4245)
    amp, ph = rng.uniform(0.4, 2.0, n), rng.uniform(0.0, 2.0 * np.pi, n)
    st = np.stack([amp * np.cos(ph), -amp * np.sin(ph)])

    def py_cb(ta, d_sgn, i):
        ta.state_data()[1, i] *= BOUNCE
        return True

    def build(variant):
        cb = {"a": hy.event_action({v: BOUNCE * v}), "b": hy.native_event_counter(), "c": py_cb}[variant]
        return hy.taylor_adaptive_batch([(x, v), (v, -x)], st, n, t_events=[hy.t_event(x, callback=cb, direction=hy.event_direction.negative)])

    return build


def outer_ss(n):
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    V = {repr(s): s for s in sys_.vars}
    st0 = configs.outer_ss_state(n, perturb=1e-6, seed=4243)
    spread = hy.taylor_adaptive_batch(sys_, st0, n, high_accuracy=True)
    spread.propagate_until(np.random.RandomState(4244).uniform(0.0, 30.0, n))
    st = np.array(spread.state)
    del spread

    def py_cb(ta, d_sgn, i):
        sd = ta.state_data()
        for r in (21, 22, 23):
            sd[r, i] *= KICK
        return True

    def build(variant):
        c_nt = hy.native_event_counter()
        cb = {"a": hy.event_action({V[k]: KICK * V[k] for k in ("vx_3", "vy_3", "vz_3")}), "b": hy.native_event_counter(), "c": py_cb}[variant]
        return hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, nt_events=[hy.nt_event(V["y_1"], c_nt), hy.nt_event(V["y_2"], c_nt)],
                                        t_events=[hy.t_event(V["y_3"], callback=cb)])

    return build


def timed_steps(ta, k):
    ta.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        ta.step()
    ta.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def terminal_events_per_step(ta, k):
    """Systems whose step ended at a terminal event (outcome = index of the event), mean over k further steps."""
    tot = 0
    for _ in range(k):
        ta.step()
        tot += int(np.sum(_outcomes(ta) >= 0))
    return tot / k


def _outcomes(ta):
    import torch

    return torch.as_tensor(ta.device_array("outcome"), device="cuda").cpu().numpy()


def measure(name, build, rounds, steps, py_steps, lines):
    print("[%s] building" % name, flush=True)
    tas = {v: build(v) for v in ("a", "b", "c")}
    assert tas["a"].event_stats["events_on_device"] and tas["b"].event_stats["events_on_device"]
    assert not tas["c"].event_stats["events_on_device"]
    # Warm-up: code objects, the buffers of the steps with events, the Taylor coefficients of the truncated steps.
    for v, k in (("a", 8), ("b", 8), ("c", 1)):
        for _ in range(k):
            tas[v].step()
    ms = {"a": [], "b": [], "c": []}
    for r in range(rounds):
        print("[%s] round %d" % (name, r), flush=True)
        for v in ("a", "b", "c"):
            ms[v].append(timed_steps(tas[v], py_steps if v == "c" else steps))
    ev = {v: terminal_events_per_step(tas[v], 2) for v in ("a", "b")}
    ta = tas["a"]
    ms0, n0 = ta.event_action_kernel_ms
    ta.set_event_timing(True)
    for _ in range(steps):
        ta.step()
    ta.set_event_timing(False)
    ms1, n1 = ta.event_action_kernel_ms
    d = (ms1 - ms0) / max(n1 - n0, 1)

    def fmt(x):
        return "%8.3f  (%s)" % (float(np.mean(x)), ", ".join("%.3f" % y for y in x))

    lines.append("%s, %d systems, stepper: %s" % (name, ta.batch_size, ta.hip_source_mode.split(":")[0][:70]))
    lines.append("  ms per step, mean over %d rounds of %d steps (the rounds); (c): %d step(s) per round" % (rounds, steps, py_steps))
    lines.append("  (a) action on the device              %s   %.0f terminal events per step" % (fmt(ms["a"]), ev["a"]))
    lines.append("  (b) counting callbacks (the floor)    %s   %.0f terminal events per step" % (fmt(ms["b"]), ev["b"]))
    lines.append("  (c) the action as a Python callback   %s" % fmt(ms["c"]))
    lines.append("  (d) hy_ev_action alone (HIP events)   %8.3f  over %d launches" % (d, n1 - n0))
    a, b = float(np.mean(ms["a"])), float(np.mean(ms["b"]))
    spread_b = float(np.max(ms["b"]) - np.min(ms["b"]))
    lines.append("  (a) - (b) - (d) = %+.3f ms; spread of (b) over the rounds %.3f ms; (c) / (a) = %.1f" % (a - b - d, spread_b, float(np.mean(ms["c"])) / a))
    lines.append("")
    return {"a": a, "b": b, "c": float(np.mean(ms["c"])), "d": d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_action_rates.log"))
    args = ap.parse_args()
    if hy.device_count() == 0:
        raise SystemExit("event_action_rates.py measures on a GPU: no HIP device visible")
    lines = ["Terminal-event actions: cost per lock-step step() (profiles/event_action_rates.py, one MI355X, one process, the",
             "variants interleaved round by round; wall clock around steps which end in a device synchronisation).", ""]
    measure("oscillators (x = 0 downwards: v <- -0.8 v)", oscillators(args.n), args.rounds, args.steps, 1, lines)
    measure("outer_ss (bench.py's events workload + Uranus crossing y = 0: v_3 <- (1 + 1e-9) v_3)", outer_ss(args.n), args.rounds, args.steps, 1, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
