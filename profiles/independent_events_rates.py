"""What batch_semantics = "independent" buys: 262 144 outer Solar Systems whose phases are spread over a synodic period of
Jupiter and Saturn, the close-encounter terminal event (squared distance - 81, direction negative, NO callback), one
horizon of half a synodic period - roughly half of the systems stop at their own encounter, the others reach the horizon.

Timed, after one untimed run of each on a copy of the ensemble (compilation, allocation):
  (a) one propagate_until() under "independent";
  (b) the workaround under the default semantics, where the first stopping event ends the call for every system:
      repeated propagate_until() calls with per-system final times - the current time for the systems which have stopped
      (outcomes and times are downloaded after every call) - until every system is done or stopped;
  (c) the same ensemble and horizon without the event: the floor.
Also: the per-step phase times of event_stats for lock-step step() of the same integrator under "reference" (the plain
stop goes through the records and the host loop) and "independent" (applied on the device).

Appends wall clock, sweeps, calls and system-steps/s of each to profiles/independent_events_rates.log, with the box and the
commit (HEYOKA_AMD_COMMIT, or git if the tree has its history); HEYOKA_AMD_RATES_LOG names a second file to append to.

usage: python profiles/independent_events_rates.py [n_systems] [horizon]"""
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402

SYNODIC = 19.86
OC = hy.taylor_outcome


def commit():
    c = os.environ.get("HEYOKA_AMD_COMMIT")
    if c:
        return c
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip() or "unknown"
    except Exception:
        return "unknown"


def close_encounter():
    x1, y1, z1, x2, y2, z2 = hy.make_vars("x_1", "y_1", "z_1", "x_2", "y_2", "z_2")
    d2 = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2) - 81.0
    return [hy.t_event(d2, direction=hy.event_direction.negative)]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    horizon = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    spread = hy.taylor_adaptive_batch(sys_, configs.outer_ss_state(n, perturb=1e-6, seed=4243), n, high_accuracy=True)
    spread.propagate_until(np.arange(n) * (SYNODIC / n))
    st = np.array(spread.state)
    del spread
    torch.cuda.empty_cache()

    def fresh(ta):
        ta.state = st
        ta.dtime = (np.zeros(n), np.zeros(n))
        if ta.with_events:
            ta.reset_cooldowns()

    res = {"n_systems": n, "horizon": horizon, "box": platform.node(), "device": torch.cuda.get_device_name(0), "commit": commit()}

    # (a) one call.
    ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, batch_semantics="independent", t_events=close_encounter())
    for timed in (False, True):
        fresh(ta)
        torch.cuda.synchronize()
        s0 = ta.event_stats["steps"]
        t0 = time.perf_counter()
        ta.propagate_until(horizon)
        oc, _, _, ns = ta.propagate_res_arrays()
        el = time.perf_counter() - t0
        sweeps = ta.event_stats["steps"] - s0
    stopped_a, t_a = oc == -1, np.array(ta.time)
    res["a_independent"] = {"wall_s": el, "calls": 1, "sweeps": int(sweeps), "system_steps": int(ns.sum()), "system_steps_per_s": float(ns.sum() / el),
                            "retired": int(ta.n_retired), "reached_the_horizon": int(np.sum(oc == int(OC.time_limit))),
                            "events_on_device": ta.event_stats["events_on_device"], "mode": ta.hip_source_mode[-80:]}
    del ta
    torch.cuda.empty_cache()

    # (b) the workaround under the default semantics.
    tb = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, t_events=close_encounter())
    for timed in (False, True):
        fresh(tb)
        torch.cuda.synchronize()
        s0 = tb.event_stats["steps"]
        t0 = time.perf_counter()
        tf = np.full(n, horizon)
        stopped = np.zeros(n, dtype=bool)
        calls, steps = 0, 0
        while True:
            tb.propagate_until(tf)
            calls += 1
            oc, _, _, ns = tb.propagate_res_arrays()
            steps += int(ns.sum())
            now = np.array(tb.time)
            new = (oc == -1) & ~stopped
            stopped |= new
            tf[new] = now[new]
            if np.all(stopped | (now == horizon)) or calls >= 1000:
                break
        el = time.perf_counter() - t0
        sweeps = tb.event_stats["steps"] - s0
    res["b_workaround_default_semantics"] = {"wall_s": el, "calls": calls, "sweeps": int(sweeps), "system_steps": steps,
                                             "system_steps_per_s": steps / el, "stopped": int(stopped.sum()),
                                             "events_on_device": tb.event_stats["events_on_device"],
                                             "same_systems_stop_as_in_a": bool(np.array_equal(stopped, stopped_a)),
                                             "same_times_as_in_a": bool(np.array_equal(np.array(tb.time), t_a))}
    del tb
    torch.cuda.empty_cache()

    # (c) the floor: no event.
    tc = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True)
    for timed in (False, True):
        fresh(tc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tc.propagate_until(horizon)
        oc, _, _, ns = tc.propagate_res_arrays()
        el = time.perf_counter() - t0
    res["c_no_event"] = {"wall_s": el, "calls": 1, "sweeps": None, "system_steps": int(ns.sum()), "system_steps_per_s": float(ns.sum() / el)}
    del tc
    torch.cuda.empty_cache()

    # Phase times of lock-step steps with the plain stop: host loop (default semantics) against the device.
    for sem in ("reference", "independent"):
        tp = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, batch_semantics=sem, t_events=close_encounter())
        for _ in range(3):
            tp.step()
        k = 8
        s0 = tp.event_stats
        tp.set_event_timing(True)
        for _ in range(k):
            tp.step()
        tp.set_event_timing(False)
        s1 = tp.event_stats
        ph = {q: round((s1[q] - s0[q]) / k, 3) for q in s1 if q.startswith("ms_")}
        ph["systems_with_events_per_step"] = (s1["systems_with_events"] - s0["systems_with_events"]) / k
        ph["events_on_device"] = s1["events_on_device"]
        res["step_phase_ms_" + sem] = ph
        del tp
        torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "independent_events_rates.log"), "a") as f:
        f.write(line + "\n")
    # (A second copy, for a run whose tree is thrown away afterwards.)
    extra = os.environ.get("HEYOKA_AMD_RATES_LOG")
    if extra:
        with open(extra, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
