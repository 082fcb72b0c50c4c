"""The generated HIP sources of the expression sections - grid observables and statistics, step actions, terminal-event
actions, the Taylor-map module - against the hashes recorded from the commit before the sections, their module caches and
the arguments of propagate_grid() were unified (tests/golden/section_sources_sha256.json). Identical source under
identical hiprtc flags is an identical code object: nothing of this needs a GPU."""
import hashlib
import json
import os

import pytest

import heyoka_amd as hy

from test_grid_observables import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "section_sources_sha256.json")
ALL = ["min", "max", "t_min", "t_max", "sum", "last", "count"]
STATISTICS = {"none": None, "all": ALL, "t_min": ["t_min"]}
MODES = {"unset": None, "registers": "registers", "staged": "staged"}


def sha(src):
    return hashlib.sha256(src.encode()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def pendulum():
    x, v = hy.make_vars("x", "v")
    return x, v, [(x, v), (v, -hy.par[0] * hy.sin(x))]


def step_actions():
    x, v, _ = pendulum()
    return {
        "assignments": hy.step_action({x: v, v: -0.5 * x}),
        "condition": hy.step_action({}, stop_when=hy.gt(x * x + v * v, 4.0)),
        "both": hy.step_action({v: 0.999 * v}, stop_when=hy.gt(x, 2.0)),
        "par_and_time": hy.step_action({v: v + hy.par[0] * hy.sin(hy.time)}, stop_when=hy.gt(hy.time * x, hy.par[0])),
    }


@pytest.mark.parametrize("stats", list(STATISTICS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_grid_sampling_source(case, ha, mode, stats, monkeypatch):
    if MODES[mode] is None:
        monkeypatch.delenv("HEYOKA_AMD_GRID_OBS", raising=False)
    else:
        monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", MODES[mode])
    sys_, obs, _, _ = case()
    src = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha, statistics=STATISTICS[stats])
    assert sha(src) == golden()["grid %s ha=%d %s %s" % (case.__name__, int(ha), mode, stats)]


@pytest.mark.parametrize("name", ["assignments", "condition", "both", "par_and_time"])
def test_step_action_source(name):
    assert sha(hy.step_action_source(pendulum()[2], step_actions()[name])) == golden()["step_action " + name]


def event_action_integrator():
    x, v, sys_ = pendulum()
    evs = [hy.t_event(x - 1.0, callback=hy.event_action({v: -0.8 * v})),
           hy.t_event(v + hy.par[0], callback=hy.event_action({x: v * hy.cos(hy.time), v: x}))]
    return hy.taylor_adaptive_batch(sys_, None, 8, t_events=evs)


def test_event_action_source():
    assert sha(event_action_integrator().event_action_module()[0]) == golden()["event_action two_events"]


def variational_integrator():
    return hy.taylor_adaptive_batch(hy.var_ode_sys(pendulum()[2], hy.var_args.vars, 1), None, 8)


def test_taylor_map_source():
    assert sha(variational_integrator().taylor_map_module()[0]) == golden()["taylor_map pendulum_vars_1"]
