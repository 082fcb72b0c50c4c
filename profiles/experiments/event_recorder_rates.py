"""Cost of recording events on the device, on the events workload of `bench.py --full`: 1 048 576 outer-Solar-System
systems spread over 30 yr of their orbits, lock-step step() with Jupiter and Saturn crossing the plane y = 0 as
non-terminal events (~170 000 events per step).

ms per step for (a) the library's counting callbacks - the floor: the same step without a log -, (b) recording callbacks
with the state columns, (c) recording callbacks without them, (d) Python callbacks which append the same header data (the
only way to get it before the event log). Prints one JSON line.

usage: python profiles/experiments/event_recorder_rates.py [n_systems] [timed steps]"""
import json
import sys
import time

import numpy as np
import torch

import heyoka_amd as hy
from heyoka_amd import configs


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
    n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st0 = configs.outer_ss_state(n, perturb=1e-6, seed=4243)
    rng = np.random.RandomState(4244)
    spread = hy.taylor_adaptive_batch(sys_, st0, n, high_accuracy=True)
    spread.propagate_until(rng.uniform(0.0, 30.0, n))
    st = np.array(spread.state)
    del spread
    torch.cuda.empty_cache()
    y1, y2 = hy.make_vars("y_1", "y_2")
    res = {}
    ref_state = None
    for name in ("counters", "recorders_with_states", "recorders_without_states", "python_callbacks"):
        rows = []
        if name == "counters":
            cbs = [hy.native_event_counter(), hy.native_event_counter()]
        elif name == "python_callbacks":
            cbs = [lambda ta, t, d, i, k=k: rows.append((i, 1, k, d, t)) for k in range(2)]
        else:
            cbs = [hy.native_event_recorder(), hy.native_event_recorder()]
        ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, nt_events=[hy.nt_event(y1, cbs[0]), hy.nt_event(y2, cbs[1])])
        if name == "recorders_without_states":
            ta.event_log_states = False
        warm, timed = (8, n_steps) if name != "python_callbacks" else (2, 2)
        if name.startswith("recorders"):
            # (Room for the rows of all the steps: no growth of the log inside the timed steps.)
            ta.event_log_reserve(int(0.6 * n) * (warm + 2 * timed + 1))

        def count():
            if name.startswith("recorders"):
                return ta.event_log_size
            return len(rows) if name == "python_callbacks" else sum(c.value for c in cbs)

        for _ in range(warm):
            ta.step()
        torch.cuda.synchronize()
        n_ev0 = count()
        t0 = time.perf_counter()
        for _ in range(timed):
            ta.step()
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / timed
        n_ev1 = count()
        r = {"ms_per_step": el * 1e3, "events_per_step": (n_ev1 - n_ev0) / timed, "timed_steps": timed,
             "mode": ta.hip_source_mode[-80:]}
        if name.startswith("recorders"):
            r["rows_per_s"] = r["events_per_step"] / el
            r["row_doubles"] = ta.event_log_row_size
            r["log_capacity_rows"] = ta.event_log_capacity
        if name != "python_callbacks":
            # Phase split (a synchronisation after every phase): stepper, detection, bookkeeping, state update + log.
            # Taken on a copy of the state of the timed run, so that the comparison of the states below is not disturbed.
            final_state = np.array(ta.state)
            s0 = ta.event_stats
            ta.set_event_timing(True)
            for _ in range(timed):
                ta.step()
            ta.set_event_timing(False)
            s1 = ta.event_stats
            r["phase_ms_per_step"] = {k: round((s1[k] - s0[k]) / timed, 3) for k in s1 if k.startswith("ms_")}
        if name == "counters":
            ref_state = final_state
        elif name != "python_callbacks":
            r["state_equals_counters_run"] = bool(np.array_equal(final_state, ref_state))
        res[name] = r
        del ta
        torch.cuda.empty_cache()
    a, b, c, d = (res[k]["ms_per_step"] for k in ("counters", "recorders_with_states", "recorders_without_states", "python_callbacks"))
    res["summary"] = {"n_systems": n, "a_counters_ms": a, "b_recorders_states_ms": b, "c_recorders_headers_ms": c,
                      "d_python_callbacks_ms": d, "b_over_a": b / a, "d_over_b": d / b,
                      "b_rows_per_s": res["recorders_with_states"]["rows_per_s"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
