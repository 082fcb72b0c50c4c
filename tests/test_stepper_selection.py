"""Which stepper emit_hip_module() selects, one small system per rung of its ladder (hip_emit_select.cpp): the
first attempt, linearised accelerations, state-variable aliases, padded clusters, unit scalings, private cluster inputs,
block mode with externalised scalings, the multi-class plan and the generic fallbacks. The selection reacts to the typed
reason of a refusal (refusal_code), the notes carry its text: the start of hip_source_mode and the note of the rewrite are
pinned per case, and for the fallbacks the whole accumulated text behind "cluster mode not applicable: " - every attempt
which was made, in order, with the reason it was refused for. Generation and hiprtc need no GPU."""
import pytest

import heyoka_amd as hy
from heyoka_amd import configs
from heyoka_amd import mixed_models as mm

from test_batch_independence import _env, tan_system
from test_models import _fixed_centres_special

N = 8
M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
HISTORY = "a state variable is a history operand of a nonlinear function"


def _centres(nc):
    masses, positions = _fixed_centres_special(nc)
    return hy.model.fixed_centres(Gconst=1.0, masses=masses, positions=positions)


# name -> sys: the system; kw: keyword arguments of the integrator; env: developer switches; start: how hip_source_mode
# begins; note: the note of the rung which served the system; tail (generic fallbacks only): the whole text behind
# "cluster mode not applicable: ".
CASES = {
    "unit_scalings_padded_4": dict(sys=lambda: hy.model.nbody(4, masses=[1.0, 2.0, 1.0, 0.0]), kw=dict(high_accuracy=True),
                                   start="cluster mode v3",
                                   note="; 2 members added to the internal program (unit scalings of elided factors, padding)"),
    "unit_scalings_padded_6": dict(sys=lambda: hy.model.nbody(6, masses=[1.0, 1.0, 1.0, 1.0, 0.0, 0.0]), start="cluster mode:",
                                   note="; 6 members added to the internal program (unit scalings of elided factors, padding)"),
    "padded_par_masses": dict(sys=lambda: hy.model.nbody(6, masses=[hy.par[i] for i in range(4)], Gconst=G), start="cluster mode v2",
                              note="; clusters of 32 missing members padded to the shape of the largest one"),
    "private_inputs_cluster": dict(sys=lambda: _centres(12), start="cluster mode v2",
                                   note="; internal program with private coordinate differences per cluster (4 members more than the decomposition)"),
    "private_inputs_block": dict(sys=lambda: _centres(70), start="block",
                                 note="; internal program with private coordinate differences per cluster (4 members more than the decomposition)"),
    "state_aliases": dict(sys=lambda: hy.model.np1body(6, masses=M, Gconst=G), start="cluster mode v2",
                          note="; state variables in history-operand position aliased by u variables"),
    "no_state_aliases": dict(sys=lambda: hy.model.np1body(6, masses=M, Gconst=G), env={"HEYOKA_AMD_NO_STATE_ALIASES": "1"},
                             start="table mode (staged)", tail=HISTORY + "; multi-class plan: " + HISTORY),
    "no_multi_class": dict(sys=lambda: mm.sine_lattice(hy, 16), env={"HEYOKA_AMD_MULTI_CLASS": "0"}, start="table mode (staged)",
                           tail=HISTORY + "; with state-variable aliases: clusters are not isomorphic (different sizes)"),
    "unrolled": dict(sys=lambda: tan_system(hy), start="unrolled",
                     tail=HISTORY + "; with state-variable aliases: clusters at different dependency levels"),
    "linearised": dict(sys=lambda: hy.model.nbody(6), start="cluster mode v5",
                       note="; accelerations rewritten as flat sums of scaled pair products in the internal program"),
    "no_linearised_sums": dict(sys=lambda: hy.model.nbody(6), env={"HEYOKA_AMD_NO_LINEARISED_SUMS": "1"}, start="cluster mode:",
                               note=" (pipelined cluster kernel not applicable: glue nodes of one group with different state-variable chains)"),
    "externalised_scalings": dict(sys=lambda: hy.model.nbody(12, masses=[1.0 + 0.125 * i for i in range(12)]), start="block",
                                  note="; scalings of the pair products moved out of the clusters in the internal program",
                                  also="v2 cluster phase"),
}
FALLBACK = "cluster mode not applicable: "


def build(name):
    case = CASES[name]
    with _env(case.get("env")):
        return hy.taylor_adaptive_batch(case["sys"](), None, N, **case.get("kw", {}))


@pytest.mark.parametrize("name", list(CASES))
def test_stepper_selected_per_rung_of_the_ladder(name):
    case = CASES[name]
    logs = []
    hy.set_log_callback(lambda lvl, msg: logs.append(msg))
    try:
        hy.set_logger_level_debug()
        mode = build(name).hip_source_mode
    finally:
        hy.set_logger_level_warn()
        hy.set_log_callback(None)
    print(mode)
    # ("<kind> [lanes per system: ..., statements: ...] <notes>": the notes begin with what the generator says of its kernel.)
    notes = mode.split("] ", 1)[1]
    assert mode.startswith(case["start"]) or notes.startswith(case["start"]), mode
    assert case.get("also", "") in mode, mode
    generic = [m for m in logs if "runs on a generic stepper instead of a wave-cluster kernel" in m]
    if "tail" in case:
        assert FALLBACK in mode, mode
        assert mode[mode.index(FALLBACK) + len(FALLBACK):] == case["tail"], mode
        assert len(generic) == 1, logs
    else:
        assert case["note"] in mode and FALLBACK not in mode, mode
        assert generic == [], generic
