"""GPU tests: every row of tests/order_cases.py - every family of steppers at Taylor orders other than the default 20, at the
lowest order of every layout the order makes the planners pick - against the oracle, at the tolerances of the families' own
parity tests (tests/test_batch_independence.py, tests/test_gpu_parity.py). What the CPU half cannot see is here: the LDS
sizes next to the limit of a CU, the jets in global scratch with their fences through memory, the builds which spill, and
the kernels behind the stepper which carry the order as well - the post-step kernel of propagate_grid(), the continuous
output, update_d_output() and the event polynomials.

n = min(2 S + 1, 65) systems of the family's own pool (S: the systems of a wavefront or workgroup; the last one is ragged).
Every test prints the measured errors in eps (pytest -s; profiles/order_sweep.log keeps a run)."""
import numpy as np
import pytest

import heyoka_amd as hy
import heyoka_oracle as ho
from heyoka_amd import codegen_check
from conftest import EPS

import order_cases as oc
import test_batch_independence as tbi
from test_gpu_parity import rel_err
from test_grid_parity import row_rel_err as grid_row_rel_err

pytestmark = pytest.mark.gpu

OC = hy.taylor_outcome


def _inputs(fam, n):
    st, pars, t0 = fam["pool"](n)
    t0v = np.zeros(n) if t0 is None else np.asarray(t0, dtype=np.float64)
    return dict(st=np.ascontiguousarray(st), pars=pars, t0=t0, t0v=t0v,
                tf=t0v + fam["t_end"] * 0.25 * np.random.RandomState(1).uniform(0.5, 1.5, n))


def _kw(inp):
    kw = {}
    if inp["pars"] is not None:
        kw["pars"] = np.ascontiguousarray(inp["pars"])
    if inp["t0"] is not None:
        kw["time"] = np.ascontiguousarray(inp["t0"])
    return kw


def _step_rec(rec, tag, sr):
    rec[tag + " outcome"] = np.array([int(o) for o, _ in sr], dtype=np.int64)
    rec[tag + " h"] = np.array([h for _, h in sr])


def _run_oracle(case, fam, inp, n):
    """(a) one step with all Taylor coefficients, (b) one backward step and one step with per-system limits - half the first
    step for the odd systems, 1e3 times it for the even ones, zero for system 0 -, (c) on a fresh integrator propagate_until()
    to per-system times."""
    family, order = case[0], case[1]
    kw = dict(fam.get("okw", {}), tol=oc.tol_for_order(order), **_kw(inp))
    log = []

    def fresh():
        if fam.get("events"):
            return ho.OracleEventIntegrator(fam["sys"](ho), inp["st"], n, **tbi._outer_ss_events(ho, log), **kw)
        return ho.OracleIntegrator(fam["sys"](ho), inp["st"], n, **kw)

    ora = fresh()
    assert ora.order == order
    dim = inp["st"].shape[0]
    o = {}
    ora.step(wtc=True)
    _step_rec(o, "step 1", ora.step_res)
    o["step 1 state"] = ora.state.reshape(dim, n).copy()
    o["step 1 Taylor coefficients"] = ora.tc.reshape(dim, order + 1, n).copy()
    lims = np.where(np.arange(n) % 2 == 1, 0.5, 1e3) * np.abs(o["step 1 h"])
    lims[0] = 0.0
    o["lims"] = lims
    ora.step(backward=True)
    _step_rec(o, "backward step", ora.step_res)
    ora.step(max_delta_ts=lims)
    _step_rec(o, "limited step", ora.step_res)
    # (From the initial time: the current time then has no low part and the final times are reached exactly.)
    ora = fresh()
    ora.propagate_until(inp["tf"])
    o["propagate_until state"] = ora.state.reshape(dim, n).copy()
    o["propagate_until time hi"], o["propagate_until time lo"] = ora.time_hi.copy(), ora.time_lo.copy()
    o["propagate_until outcome"] = np.array([int(r[0]) for r in ora.prop_res], dtype=np.int64)
    o["propagate_until steps"] = np.array([int(r[3]) for r in ora.prop_res], dtype=np.int64)
    o["events"] = sorted(log, key=lambda e: e[0])
    if fam.get("mixed"):
        # (The lanes on which the oracle's two orders of the operations agree on h: assert_close_to_oracle().)
        okw = {k: v for k, v in kw.items() if k != "compact_mode"}
        oc_ = ho.OracleIntegrator(fam["sys"](ho), inp["st"], n, compact_mode=True, **okw)
        oc_.step()
        h_c = np.array([h for _, h in oc_.step_res])
        o["well"] = np.abs(h_c - o["step 1 h"]) / np.abs(o["step 1 h"]) <= 1e3 * EPS
    return o


def _run_product(case, inp, n, lims):
    family, order = case[0], case[1]
    log = []

    def fresh():
        ta = oc.construct(family, order, n, inp["st"], event_log=log, **_kw(inp))
        oc.check_mode(case, ta.hip_source_mode)
        assert ta.order == order
        return ta

    ta = fresh()
    rec = {}
    ta.step(write_tc=True)
    _step_rec(rec, "step 1", ta.step_res)
    rec["step 1 state"] = np.asarray(ta.state).copy()
    rec["step 1 Taylor coefficients"] = np.asarray(ta.tc).copy()
    ta.step_backward()
    _step_rec(rec, "backward step", ta.step_res)
    ta.step(max_delta_t=lims)
    _step_rec(rec, "limited step", ta.step_res)
    ta = fresh()
    ta.propagate_until(inp["tf"])
    oc_, mn, mx, ns = ta.propagate_res_arrays()
    hi, lo = ta.dtime
    rec.update({"propagate_until state": np.asarray(ta.state).copy(), "propagate_until time hi": hi.copy(), "propagate_until time lo": lo.copy(),
                "propagate_until outcome": np.asarray(oc_, dtype=np.int64).copy(), "propagate_until steps": np.asarray(ns).astype(np.int64),
                "propagate_until min |h|": np.asarray(mn).copy(), "propagate_until max |h|": np.asarray(mx).copy()})
    return rec, ta, sorted(log, key=lambda e: e[0])


def _compare_events(label, ev, ev_o):
    """Systems, events, directions and order exact; times at the 1e-12 of test_events_batch_vs_oracle."""
    assert [(e[0], e[1], e[3]) for e in ev] == [(e[0], e[1], e[3]) for e in ev_o], label
    assert len(ev_o) > 0, label
    dt = max(abs((a[2] - b[2]) + (a[4] - b[4])) for a, b in zip(ev, ev_o))
    print("[%s] %d events, largest difference of an event time %.3g" % (label, len(ev_o), dt))
    assert dt <= 1e-12, label


@pytest.mark.parametrize("case", oc.ORDER_CASES, ids=oc.case_id)
def test_order_case_vs_oracle(case):
    """(a) One step with all Taylor coefficients: outcomes exact, h and coefficients to 1e6 eps, state to 1e5 eps. (b) A
    backward step and a step with per-system limits, one of them zero: outcomes exact, h to rtol 1e-9. (c) propagate_until()
    to per-system final times: outcomes exact; final times exact (hi == tf bit for bit) on every system where the oracle's
    are - all but one system of one row, which is held to 4 eps on the pair (hi, lo) -; step counts within 1 and different on
    at most 2 systems, states at the family's tolerance; the event log of the stepper with events against the oracle's.
    (d) Where the build spills registers: a second fresh integrator gives the same results bit for bit."""
    family, order = case[0], case[1]
    fam = tbi.FAMILIES[family]
    probe = oc.construct(family, order, 1)
    oc.check_mode(case, probe.hip_source_mode)
    mode = probe.hip_source_mode
    S = oc.systems_per_unit(mode)
    res = codegen_check.kernel_resources(probe.code_object)
    del probe
    n = 3 if family == "block_v2_nbody64" else min(2 * S + 1, 65)
    label = oc.case_id(case)
    print("\n[%s] %s; S = %d, %d systems; vgpr_spill %d, scratch_bytes_per_lane %d, lds_bytes %d"
          % (label, ", ".join(map(str, oc.layout_key(mode))), S, n, res["vgpr_spill"],
             res["scratch_bytes_per_lane"], res["lds_bytes"]))
    inp = _inputs(fam, n)
    o = _run_oracle(case, fam, inp, n)
    rec, ta, ev = _run_product(case, inp, n, o["lims"])
    idx = np.arange(n)
    assert not any(np.isnan(v).any() for v in rec.values()), label
    # (a) and the states of (c): the families' own comparison (the events of the stepper with events: below, at 1e-12).
    tbi.assert_close_to_oracle(label, dict(fam, events=False), rec, ev, o, idx)
    # (b)
    for tag in ("backward step", "limited step"):
        assert np.array_equal(rec[tag + " outcome"], o[tag + " outcome"]), (label, tag)
        assert np.allclose(rec[tag + " h"], o[tag + " h"], rtol=1e-9, atol=0), (label, tag)
    assert np.all(rec["backward step h"] < 0) and rec["limited step h"][0] == 0.0
    clamped = rec["limited step outcome"] == int(OC.time_limit)
    assert clamped[0] and np.all(clamped[1::2]) and not np.any(clamped[2::2]), label
    # (c)
    assert np.all(rec["propagate_until outcome"] == int(OC.time_limit)), label
    # The final times: EXACT - the high part of the time IS the final time, bit for bit - on every system on which the oracle's
    # is (the propagation starts from the initial time: no low part to begin with). The last step is clamped to the high part
    # of the remaining time and the new time is a double-length sum, so where the time before it has a low part the
    # reference's high part can end an ulp off the final time with the rest in the low part: the oracle's does on one system
    # of one row (table_hbm, order 15). Those systems alone - the oracle's inexact ones - are held to the criterion of
    # tests/test_batch_independence.py instead: the pair (hi, lo) within 4 eps of the final time (and hi within 2 ulp of the
    # oracle's: assert_close_to_oracle() above).
    tf, hi, lo, hi_o = inp["tf"], rec["propagate_until time hi"], rec["propagate_until time lo"], o["propagate_until time hi"]
    exact = hi_o == tf
    print("[%s] final times: the oracle's hi is the final time bit for bit on %d of %d systems; the kernel's on %d"
          % (label, np.count_nonzero(exact), n, np.count_nonzero(hi == tf)))
    assert np.count_nonzero(~exact) <= 1, label
    assert np.array_equal(hi[exact], tf[exact]), (label, np.flatnonzero(hi != tf))
    t_err = np.abs((hi - tf) + lo)
    assert np.all(t_err[~exact] <= 4.0 * EPS * np.maximum(1.0, np.abs(tf[~exact]))), label
    dn = np.abs(rec["propagate_until steps"] - o["propagate_until steps"])
    assert dn.max() <= 1 and np.count_nonzero(dn) <= 2, (label, dn)
    if fam.get("events"):
        _compare_events(label, ev, o["events"])
    # (d)
    if res["vgpr_spill"] > 0:
        rec2, tb, ev2 = _run_product(case, inp, n, o["lims"])
        assert tb.hip_source == ta.hip_source
        for key, val in rec.items():
            assert np.array_equal(val, rec2[key]), (label, "second run", key)
        assert ev == ev2, label
        print("[%s] %d spilled registers: a second fresh integrator gives the same %d arrays bit for bit" % (label, res["vgpr_spill"], len(rec)))


# ---- (e) the kernels behind the stepper ----
@pytest.mark.parametrize("order", [3, 15, 22])
@pytest.mark.parametrize("which", ["v5", "unrolled"])
def test_post_step_kernels_at_other_orders(which, order):
    """The outer Solar System on the one-lane-per-pair stepper and the tan system on the straight-line stepper.
    propagate_grid() over 9 points per system: with and without a callback (a sweep per step / one launch per grid
    interval where the stepper has it) bit for bit the same, and to 1e6 eps of the oracle's grid; the continuous output of
    propagate_until() at 5 of the grid times against the oracle's dense output there (its grid samples: the same steps, only
    the last one is clamped); update_d_output() at a time inside the step just taken against the oracle's dense output."""
    family = "v5" if which == "v5" else "unrolled"
    fam = tbi.FAMILIES[family]
    want = "mode v5" if which == "v5" else "unrolled"
    n = 9 if which == "v5" else 65
    inp = _inputs(fam, n)
    st = inp["st"]
    dim = st.shape[0]
    # (7.5 years of the outer Solar System: 10 .. 15 steps; 4 time units of the tan system, whose steps are about 0.5 long.)
    span = (0.25 if which == "v5" else 5.0) * fam["t_end"] * (1.0 + 0.03 * (np.arange(n) % 7))
    grid = np.linspace(0.0, 1.0, 9)[:, None] * span[None, :]
    label = "%s, order %d" % (family, order)
    err = (lambda a, b: float(rel_err(a, b))) if fam.get("floor_at_one") else grid_row_rel_err

    def fresh():
        ta = oc.construct(family, order, n, st)
        assert want in ta.hip_source_mode and ta.order == order, ta.hip_source_mode
        return ta

    okw = dict(fam.get("okw", {}), tol=oc.tol_for_order(order))
    ora = ho.OracleIntegrator(fam["sys"](ho), st, n, **okw)
    _, out_o = ora.propagate_grid(grid)
    ta = fresh()
    _, out = ta.propagate_grid(grid)
    tb = fresh()
    calls = []
    _, out_cb = tb.propagate_grid(grid, callback=lambda t: calls.append(1) or True)
    assert len(calls) >= max(r[3] for r in ta.propagate_res)
    assert np.array_equal(out, out_cb) and np.array_equal(ta.state, tb.state) and ta.propagate_res == tb.propagate_res, label
    assert [int(r[0]) for r in ta.propagate_res] == [int(r[0]) for r in ora.prop_res] == [int(OC.time_limit)] * n, label
    assert not np.isnan(out).any() and not np.isnan(out_o).any(), label
    dn = np.abs(np.array([int(r[3]) for r in ta.propagate_res]) - np.array([int(r[3]) for r in ora.prop_res]))
    e_grid, e_st = err(out, out_o) / EPS, err(np.asarray(ta.state), ora.state.reshape(dim, n)) / EPS
    assert dn.max() <= 1 and np.count_nonzero(dn) <= 2, (label, dn)
    # Continuous output at 5 of the grid times.
    tc_ = fresh()
    co, _ = tc_.propagate_until(grid[-1].copy(), c_output=True)
    e_co = 0.0
    for j in (1, 3, 4, 6, 8):
        e_co = max(e_co, err(np.asarray(co(grid[j].copy()))[None], out_o[j][None]) / EPS)
    # update_d_output() in the middle of the first step.
    td = fresh()
    ord_ = ho.OracleIntegrator(fam["sys"](ho), st, n, **okw)
    td.step(write_tc=True)
    ord_.step(wtc=True)
    h_o = np.array([h for _, h in ord_.step_res])
    d = td.update_d_output(0.5 * h_o)
    d_o = np.stack([ord_._dense(i, 0.5 * h_o[i]) for i in range(n)], axis=1)
    e_d = err(d[None], d_o[None]) / EPS
    print("\n[%s, post-step kernels vs oracle, eps] grid samples %.3g, final states %.3g (%d .. %d steps, %d step counts differ), "
          "continuous output %.3g, update_d_output %.3g" % (label, e_grid, e_st, min(r[3] for r in ora.prop_res),
                                                            max(r[3] for r in ora.prop_res), np.count_nonzero(dn), e_co, e_d))
    assert e_grid <= 1e6 and e_st <= 1e6 and e_co <= 1e6 and e_d <= 1e6, label


# ---- (f) event polynomials ----
def _tan_events(m, log):
    """One non-terminal and one terminal event on the tan system (the events of 'events:unrolled' in
    tests/stepper_source_corpus.py); the terminal event's callback keeps the system going."""
    x, y = tbi._vars(m, "x", "y")

    def te(ta, d, i):
        hi, lo = (ta.time_hi, ta.time_lo) if m is ho else ta.dtime
        log.append((int(i), 1, float(hi[i]), int(d), float(lo[i])))
        return True

    return dict(nt_events=[m.nt_event(x - 0.1, lambda ta, t, d, i: log.append((int(i), 0, float(t), int(d), 0.0)))],
                t_events=[m.t_event(x + y, te)])


@pytest.mark.parametrize("order", [3, 8, 22])
@pytest.mark.parametrize("stepper", ["unrolled", "staged", "table_hbm"])
def test_tan_system_events_at_other_orders(stepper, order):
    """The event polynomials carry the order as well (their coefficients, the root isolation, the lists of detected events
    sized from it): the tan system with one non-terminal and one terminal event on the straight-line and the two table
    steppers, propagated to per-system times - the event log against the oracle's: systems, events, directions and order
    exact, times to 1e-12; outcomes exact, states to 1e6 eps."""
    fam = tbi.FAMILIES["unrolled"]
    n = 65
    inp = _inputs(fam, n)
    # (Five times the horizon of the family: x decays through 0.1 on the systems which start above it.)
    tf = 5.0 * fam["t_end"] * np.random.RandomState(1).uniform(0.5, 1.5, n)
    kw = {} if stepper == "unrolled" else {"emitter": "table"}
    want = {"unrolled": "unrolled", "staged": "table mode (staged)", "table_hbm": "tape in HBM"}[stepper]
    log, log_o = [], []
    with tbi._env({"HEYOKA_AMD_TABLE_LDS": "0"} if stepper == "table_hbm" else None):
        ta = hy.taylor_adaptive_batch(tbi.tan_system(hy), inp["st"], n, tol=oc.tol_for_order(order), **_tan_events(hy, log), **kw)
    assert want in ta.hip_source_mode and ta.order == order, ta.hip_source_mode
    ora = ho.OracleEventIntegrator(tbi.tan_system(ho), inp["st"], n, tol=oc.tol_for_order(order), **_tan_events(ho, log_o))
    ta.propagate_until(tf)
    ora.propagate_until(tf)
    label = "tan system with events, %s, order %d" % (stepper, order)
    assert [int(r[0]) for r in ta.propagate_res] == [int(r[0]) for r in ora.prop_res], label
    _compare_events(label, sorted(log, key=lambda e: e[0]), sorted(log_o, key=lambda e: e[0]))
    e_st = float(rel_err(np.asarray(ta.state), ora.state.reshape(2, n))) / EPS
    print("[%s] state %.3g eps" % (label, e_st))
    assert e_st <= 1e6, label
