"""Cost of the event-log observables in the protocol of profiles/event_recorder_rates.log: the events
workload of `bench.py --full` - 1 048 576 outer-Solar-System systems spread over 30 yr of their orbits, lock-step step()
with Jupiter and Saturn crossing the plane y = 0 as non-terminal events.

ms per lock-step step, median of three windows with their spread, for (a) counting callbacks, (c) recorders without
states, (b) recorders with the 36 state columns, (o6) observables = one squared pair distance (6 state rows read), (o36)
observables = the energy (36 rows read); the bytes a step appends to the log; and the row kernel alone - hy_dout_rows /
hy_obs_rows is the one thing the "state update + log" phase of a variant does beyond the same phase of (c), so its time is
that difference of the phase split (a stream synchronisation after every phase). Prints one JSON line.

usage: python profiles/event_observables_rates.py [n_systems] [steps per window]"""
import json
import statistics
import sys
import time

import numpy as np
import torch

import heyoka_amd as hy
from heyoka_amd import configs

VARIANTS = ("counters", "recorders_without_states", "recorders_with_states", "observables_pair_distance", "observables_energy")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
    n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    sys_ = hy.model.nbody(6, masses=M, Gconst=G)
    st0 = configs.outer_ss_state(n, perturb=1e-6, seed=4243)
    rng = np.random.RandomState(4244)
    spread = hy.taylor_adaptive_batch(sys_, st0, n, high_accuracy=True)
    spread.propagate_until(rng.uniform(0.0, 30.0, n))
    st = np.array(spread.state)
    del spread
    torch.cuda.empty_cache()
    var = {repr(e): e for e in sys_.vars}
    y1, y2 = var["y_1"], var["y_2"]
    obs = {"observables_pair_distance": [hy.sum([(var["%s_1" % c] - var["%s_2" % c]) * (var["%s_1" % c] - var["%s_2" % c]) for c in "xyz"])],
           "observables_energy": [hy.model.nbody_energy(6, masses=M, Gconst=G)]}
    res = {}
    ref_state = None
    warm, windows = 8, 3
    for name in VARIANTS:
        rec = name != "counters"
        cbs = [hy.native_event_recorder() if rec else hy.native_event_counter() for _ in range(2)]
        ta = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=True, nt_events=[hy.nt_event(y1, cbs[0]), hy.nt_event(y2, cbs[1])])
        if name == "recorders_without_states":
            ta.event_log_states = False
        if name in obs:
            ta.event_log_observables = obs[name]
        if rec:
            # (Room for the rows of all the steps: no growth of the log inside the timed steps.)
            ta.event_log_reserve(int(0.25 * n) * (warm + 2 * windows * n_steps + 1))
        count = (lambda: ta.event_log_size) if rec else (lambda: sum(c.value for c in cbs))
        for _ in range(warm):
            ta.step()
        torch.cuda.synchronize()
        n_ev0 = count()
        ms = []
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(n_steps):
                ta.step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / n_steps * 1e3)
        ev = (count() - n_ev0) / (windows * n_steps)
        r = {"ms_per_step_windows": [round(x, 4) for x in ms], "ms_per_step": statistics.median(ms), "spread_ms": max(ms) - min(ms),
             "events_per_step": ev, "mode": ta.hip_source_mode[-80:]}
        if rec:
            r["row_doubles"] = ta.event_log_row_size
            r["log_bytes_per_step"] = ev * ta.event_log_row_size * 8
        final_state = np.array(ta.state)
        # Phase split, per window as well: stepper, detection, bookkeeping, state update + log.
        ta.set_event_timing(True)
        phases = []
        for _ in range(windows):
            s0 = ta.event_stats
            for _ in range(n_steps):
                ta.step()
            s1 = ta.event_stats
            phases.append({k: (s1[k] - s0[k]) / n_steps for k in s1 if k.startswith("ms_")})
        ta.set_event_timing(False)
        r["phase_ms_per_step"] = {k: round(statistics.median(p[k] for p in phases), 4) for k in phases[0]}
        r["phase_spread_ms"] = {k: round(max(p[k] for p in phases) - min(p[k] for p in phases), 4) for k in phases[0]}
        if name == "counters":
            ref_state = final_state
        else:
            r["state_equals_counters_run"] = bool(np.array_equal(final_state, ref_state))
        res[name] = r
        del ta
        torch.cuda.empty_cache()
    base = res["recorders_without_states"]["phase_ms_per_step"]
    for name in VARIANTS[2:]:
        p = res[name]["phase_ms_per_step"]
        res[name]["row_kernel_ms"] = round(p["ms_update_records"] - base["ms_update_records"], 4)
        res[name]["stepper_store_ms"] = round(p["ms_stepper"] - base["ms_stepper"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
