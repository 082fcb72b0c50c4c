#!/usr/bin/env python
"""Fingerprints of the generated steppers, for refactors of the generators: `python tests/stepper_source_corpus.py OUT`
constructs a corpus of integrators (no GPU is needed: the generator is host code and hiprtc cross-compiles) and writes one
JSON line per entry with hip_source_mode, three hashes, lanes_per_system and the statement count as hip_source_mode prints
them. Generation and compilation are deterministic; no hash file is committed (it would have to change with every kernel
improvement): write the file at the parent commit and at the result and `diff` the two. Not collected by pytest.

What each hash is good for:
- hip_source_sha256 (the generated text): a generator this change is not meant to touch emits the same text, comments
  included - the whole line of such an entry is identical.
- device_code_sha256 (the contents of the ELF sections .text, .rodata and .note of the code object, in this order: the
  instructions, the constant tables, the kernel descriptors' metadata - registers, LDS, scratch, arguments): the check of a
  change which moves or rewrites source text and is meant to leave the machine code alone. Comments, macro names and the
  names of static symbols do not reach it.
- code_object_sha256 (the whole file): changes with any edit of the text, a comment included (the symbol hash tables
  differ), so it says no more than hip_source_sha256 unless the text is identical - then it pins the compiler.

The corpus: the families of tests/test_batch_independence.py, the block-mode generator (hip_emit_block*.cpp) on nbody(12),
nbody(64) and nbody(80) - one, four and seven rounds per lane - under every switch of HEYOKA_AMD_BLOCK_OPTS and on the
systems which keep it on its generic cluster phase, the outer Solar System under every switch of the pipelined / lane-pair / one-lane-per-pair generator
(hip_emit_cluster2*.cpp), its stepper with events under the switches of the event path, the systems which take the retries
of emit_hip_module() (block mode with and without the v2 cluster phase, linearised accelerations, multi-class plans; as
select:<case> the cases of tests/test_stepper_selection.py which take its other rungs, with their own switches), the
first wave-cluster generator with one class of clusters (cluster_kernel="v1"), and the straight-line, HBM-tape and staged
steppers with events (HY_N_EV > 0, mode 4), without compensated summation and with a fused angle reduction; as aux:<module>
the auxiliary modules which evaluate dense output from the coefficient buffer (aux_corpus())."""
import hashlib
import json
import os
import re
import struct
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.join(HERE, "emu"), os.path.join(os.path.dirname(HERE), "oracle"), os.path.dirname(HERE), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import heyoka_amd as hy  # noqa: E402
from heyoka_amd import configs  # noqa: E402
import test_batch_independence as tbi  # noqa: E402
import test_event_observables as teo  # noqa: E402
import test_stepper_selection as tss  # noqa: E402

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
    out += [family("block_v2"), family("block_centres"), family("multi_class"), family("block_v2_nbody64")]
    out += block_corpus()
    out.append(("equal_masses_linearised", lambda: hy.taylor_adaptive_batch(hy.model.nbody(6), None, N, high_accuracy=True), None))
    # The steppers with one copy of the step loop each (emit_detail::step_loop_source()).
    out += [family(n) for n in ("unrolled", "unrolled_two_waves", "unrolled_register_jets", "staged", "staged_functions", "table_hbm",
                                "table_hbm_functions")]
    out.append(("cluster_v1", lambda: outer(cluster_kernel="v1"), None))
    hbm = {"HEYOKA_AMD_TABLE_LDS": "0"}
    out.append(("events:unrolled", lambda: tan(**_tan_events()), None))
    out.append(("events:staged", lambda: outer_ev(emitter="table"), None))
    out.append(("events:table_hbm", lambda: outer_ev(emitter="table"), hbm))
    out.append(("table_hbm:high_accuracy=False", lambda: outer(emitter="table", high_accuracy=False), hbm))
    for tag, kw, env in (("unrolled", {}, None), ("staged", {"emitter": "table"}, None), ("table_hbm", {"emitter": "table"}, hbm)):
        out.append(("angle_reduce:" + tag, lambda kw=kw: fused_angle_reduce(tan(**kw), [1]), env))
    # The rungs of the selection ladder (tests/test_stepper_selection.py) which no entry above takes.
    for name in ("unit_scalings_padded_4", "unit_scalings_padded_6", "padded_par_masses", "private_inputs_cluster", "private_inputs_block",
                 "no_state_aliases", "no_multi_class", "no_linearised_sums"):
        out.append(("select:" + name, lambda name=name: tss.build(name), None))
    out += aux_corpus()
    return out


def aux_module(ta, pair):
    """A (source, code object) pair of an auxiliary module of ta, as an object with the three attributes main() reads."""
    return types.SimpleNamespace(hip_source=pair[0], code_object=pair[1], hip_source_mode=ta.hip_source_mode)


def aux_corpus():
    """The modules which evaluate dense output from the coefficient buffer next to the steppers: the companion module of the
    wave-cluster stepper with events (hy_dout_c and hy_tc_expand; with hy_ev_jets when the event equations are kept out of
    the stepper), hy_dout_rows and hy_obs_rows of the event log - on compact coefficients (outer Solar System) and on full
    ones (the pendulum of tests/test_event_observables.py), in both arithmetics and with exact divisions."""
    def log_module(make, which, obs=None):
        def build():
            ta = make()
            if obs is not None:
                ta.event_log_observables = obs()
            return aux_module(ta, (ta.event_log_source(which), ta.event_log_code_object(which)))
        return build

    def event_jets(ta):
        return aux_module(ta, ta.event_jets_module())

    def outer_rec(high_accuracy=True, **kw):
        # (The outer Solar System with recording callbacks of tests/test_event_observables.py.)
        return teo._outer_ss(high_accuracy, **kw)[0]

    def outer_obs():
        # Positions (rows derived from the velocities on compact coefficients), and a velocity on its own (a defining row).
        vx, vy = hy.make_vars("vx_2", "vy_2")
        return [teo._pair_distance2(), vx * vx + vy * vy]

    out = []
    variants = (("default", {}), ("exact_division", {"exact_division": True}), ("high_accuracy=False", {"high_accuracy": False}))
    for tag, env in (("in_stepper", None), ("no_events_in_stepper", {"HEYOKA_AMD_NO_EVENTS_IN_STEPPER": "1"})):
        for vtag, kw in variants:
            name = "%s:%s" % (tag, vtag)
            rec = lambda kw=kw: outer_rec(**kw)
            out.append(("aux:event_jets:" + name, lambda kw=kw: event_jets(outer_ev(**kw)), env))
            out.append(("aux:event_log1:" + name, log_module(rec, 1), env))
            if env is None:
                for mode in ("registers", "staged"):
                    out.append(("aux:event_log2:%s:%s" % (mode, vtag), log_module(rec, 2, outer_obs), {"HEYOKA_AMD_EVENT_OBS": mode}))
    for ha in (False, True):
        pend = lambda ha=ha: teo._cpu_ta(high_accuracy=ha)[0]
        out.append(("aux:event_log1:pendulum:high_accuracy=%s" % ha, log_module(pend, 1), None))
        for mode in ("registers", "staged"):
            out.append(("aux:event_log2:pendulum:%s:high_accuracy=%s" % (mode, ha),
                        log_module(pend, 2, lambda: teo._pendulum_obs(*hy.make_vars("x", "v"))), {"HEYOKA_AMD_EVENT_OBS": mode}))
    return out


BLOCK_SWITCHES = ("nopad", "perm", "licm", "bs=64", "M=3", "reg_high", "reg_high=2", "div", "split", "xpf", "unpacked", "noglueperm",
                  "nofuse", "dbuf", "G=1", "D=2", "D=1", "hand=2", "hoist", "keepdz", "hoist=0", "keepdz=0", "nopp", "nopp=0", "exp=1",
                  "exp=2", "exp=3", "exp=4", "exp=5", "exp=34", "nopad,licm,bs=64")


def block_corpus():
    """The block-mode generator: 66 clusters on 128 lanes (one round), 2016 on 512 (two wavefronts per SIMD, four rounds), 3160
    (seven rounds, the lean variant); the first two under every switch; what keeps nbody(12) off the v2 cluster phase."""
    def nbody(n, **kw):
        def make(**kw2):
            kw2.setdefault("high_accuracy", True)
            return hy.taylor_adaptive_batch(hy.model.nbody(n, **kw), None, N, **kw2)
        return make

    out = [("block:nbody%d" % n, nbody(n), None) for n in (12, 64, 80)]
    for n in (12, 64):
        out += [("block:nbody%d:%s" % (n, sw), nbody(n), {"HEYOKA_AMD_BLOCK_OPTS": sw}) for sw in BLOCK_SWITCHES]
    out.append(("block:nbody12:v2=0", nbody(12), {"HEYOKA_AMD_BLOCK_V2": "0"}))
    out.append(("block:nbody12:exact_division", lambda: nbody(12)(exact_division=True), None))
    out.append(("block:nbody12:high_accuracy=False", lambda: nbody(12)(high_accuracy=False), None))
    out.append(("block:nbody12:distinct_masses", nbody(12, masses=[1.0 + 0.125 * i for i in range(12)]), None))
    out.append(("block:nbody12:runtime_masses", nbody(12, masses=[hy.par[i] for i in range(12)]), None))
    out.append(("block:nbody8:emitter=block", lambda: nbody(8)(emitter="block"), None))
    return out


def tan(**kw):
    return hy.taylor_adaptive_batch(tbi.tan_system(hy), None, N, **kw)


def _tan_events():
    x, y = hy.make_vars("x", "y")
    return dict(nt_events=[hy.nt_event(x - 0.1, lambda *a: None)], t_events=[hy.t_event(x + y, lambda *a: True)])


def fused_angle_reduce(ta, idx):
    """The variant of ta's stepper with callback::angle_reducer fused in, as an object with the three attributes main() reads."""
    src, why = ta.angle_reduce_variant_source(idx)
    assert src, why
    return types.SimpleNamespace(hip_source=src, code_object=hy.hiprtc_compile(src), hip_source_mode=ta.hip_source_mode + " [angle_reduce]")


def device_code(elf):
    """The contents of the sections .text, .rodata and .note of an ELF64 (little-endian) file, concatenated in this order."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    assert elf[:6] == b"\x7fELF\x02\x01" and shentsize == 64, "not an ELF64 little-endian file"
    hdr = [struct.unpack_from("<IIQQQQ", elf, shoff + 64 * i) for i in range(shnum)]  # name, type, flags, addr, offset, size
    strtab = elf[hdr[shstrndx][4]:hdr[shstrndx][4] + hdr[shstrndx][5]]
    by_name = {strtab[h[0]:strtab.index(b"\0", h[0])].decode(): elf[h[4]:h[4] + h[5]] for h in hdr if h[1] != 8}  # (8: SHT_NOBITS)
    assert ".text" in by_name and ".note" in by_name, sorted(by_name)
    return b"".join(by_name.get(n, b"") for n in (".text", ".rodata", ".note"))


def main(path, only=""):
    sha = lambda b: hashlib.sha256(b).hexdigest()
    with open(path, "w") as f:
        for name, make, env in corpus():
            if only not in name:
                continue
            with tbi._env(env):
                ta = make()
            mode = ta.hip_source_mode
            lanes = re.search(r"lanes per system: (\d+)", mode)
            stmts = re.search(r"statements: (\d+)", mode)
            f.write(json.dumps({"entry": name, "hip_source_mode": mode, "hip_source_sha256": sha(ta.hip_source.encode()),
                                "code_object_sha256": sha(bytes(ta.code_object)),
                                "device_code_sha256": sha(device_code(bytes(ta.code_object))),
                                "lanes_per_system": int(lanes.group(1)) if lanes else None,
                                "statements": int(stmts.group(1)) if stmts else None}, sort_keys=True) + "\n")
            f.flush()
            print(name, mode.split(":")[0][-50:], flush=True)


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit("usage: stepper_source_corpus.py OUTPUT.jsonl [only the entries whose name contains this]")
    main(*sys.argv[1:])
