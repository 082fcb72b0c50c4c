#!/usr/bin/env python
"""Fingerprints of the generated steppers, for refactors of the generators: `python tests/stepper_source_corpus.py OUT`
constructs a corpus of integrators (no GPU is needed: the generator is host code and hiprtc cross-compiles) and writes one
JSON line per entry with hip_source_mode, the sha256 of hip_source and of code_object, lanes_per_system and the statement
count as hip_source_mode prints them. Generation and compilation are deterministic, so a change which is meant to leave
every kernel as it is is one after which this file is byte for byte the file of the parent commit (`diff` is the check;
no hash file is committed - it would have to change with every kernel improvement). Not collected by pytest.

The corpus: the wave-cluster families of tests/test_batch_independence.py, the outer Solar System under every switch of
the pipelined / lane-pair / one-lane-per-pair generator (hip_emit_cluster2*.cpp), its stepper with events under the
switches of the event path, and the systems which take the retries of emit_hip_module() (block mode with and without the
v2 cluster phase, linearised accelerations, multi-class plans)."""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.join(HERE, "emu"), os.path.join(os.path.dirname(HERE), "oracle"), os.path.dirname(HERE), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402
import test_batch_independence as tbi  # noqa: E402

M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
N = 64


def outer(**kw):
    kw.setdefault("high_accuracy", True)
    return hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), None, N, **kw)


def outer_ev(**kw):
    return outer(**tbi._outer_ss_events(hy, []), **kw)


def family(name):
    fam = tbi.FAMILIES[name]

    def make():
        kw = dict(fam.get("kw", {}))
        if fam.get("events"):
            kw.update(tbi._outer_ss_events(hy, []))
        return hy.taylor_adaptive_batch(fam["sys"](hy), None, N, **kw)

    return "family:" + name, make, fam.get("env")


def corpus():
    """(name, constructor, environment) per entry."""
    out = [family(n) for n in ("v5", "v5_32_lanes", "v5_8_lanes_lds_jets", "v5_16_lanes_lds_jets", "v5_events", "v3", "v3_64_lanes",
                               "v2", "v2_aliased")]
    for f in ("nofrx", "nobkslab", "nowide", "novx", "nostoreplace", "frxlds", "nopack2", "norx", "nomsq", "nosc", "notailrd",
              "nofrx+norx", "nofrx+nostoreplace", "bankdbg"):
        out.append(("v5_opts:" + f, outer, {"HEYOKA_AMD_V5_OPTS": f}))
    for p in "0123":
        out.append(("v5_prio:" + p, outer, {"HEYOKA_AMD_V5_PRIO": p}))
    out.append(("no_refill", outer, {"HEYOKA_AMD_NO_REFILL": "1"}))
    # (One of the variants of profiles/experiments/sensitivity.py.)
    out.append(("v5_pad:0:0:2:0:0", outer, {"HEYOKA_AMD_V5_PAD": "0:0:2:0:0"}))
    out.append(("exact_division", lambda: outer(exact_division=True), None))
    out.append(("high_accuracy=False", lambda: outer(high_accuracy=False), None))
    out.append(("tol=1e-9", lambda: outer(tol=1e-9), None))
    out.append(("runtime_masses",
                lambda: hy.taylor_adaptive_batch(hy.model.nbody(6, masses=[hy.par[i] for i in range(6)]), None, N, high_accuracy=True), None))
    out.append(("events:default", outer_ev, None))
    for tag, env in (("v5_events=0", {"HEYOKA_AMD_V5_EVENTS": "0"}), ("compact_tc=0", {"HEYOKA_AMD_COMPACT_TC": "0"}),
                     ("no_events_in_stepper", {"HEYOKA_AMD_NO_EVENTS_IN_STEPPER": "1"}), ("no_pair_events", {"HEYOKA_AMD_NO_PAIR_EVENTS": "1"}),
                     ("one_lane=0", {"HEYOKA_AMD_ONE_LANE": "0"}), ("one_lane=0,pair_split=0", {"HEYOKA_AMD_ONE_LANE": "0", "HEYOKA_AMD_PAIR_SPLIT": "0"})):
        out.append(("events:" + tag, outer_ev, env))
    # The dispatch of emit_hip_module().
    out += [family("block_v2"), family("block_centres"), family("multi_class")]
    out.append(("equal_masses_linearised", lambda: hy.taylor_adaptive_batch(hy.model.nbody(6), None, N, high_accuracy=True), None))
    return out


def main(path):
    sha = lambda b: hashlib.sha256(b).hexdigest()
    with open(path, "w") as f:
        for name, make, env in corpus():
            with tbi._env(env):
                ta = make()
            mode = ta.hip_source_mode
            lanes = re.search(r"lanes per system: (\d+)", mode)
            stmts = re.search(r"statements: (\d+)", mode)
            f.write(json.dumps({"entry": name, "hip_source_mode": mode, "hip_source_sha256": sha(ta.hip_source.encode()),
                                "code_object_sha256": sha(bytes(ta.code_object)),
                                "lanes_per_system": int(lanes.group(1)) if lanes else None,
                                "statements": int(stmts.group(1)) if stmts else None}, sort_keys=True) + "\n")
            f.flush()
            print(name, mode.split(":")[0][-50:], flush=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: stepper_source_corpus.py OUTPUT.jsonl")
    main(sys.argv[1])
