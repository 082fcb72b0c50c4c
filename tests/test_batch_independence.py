"""Batch-size independence of every stepper: the integration of a system depends only on that system's own state,
parameters, time and limits, so its results are the same BIT FOR BIT whatever the batch size, wherever in the batch the
system sits and whoever its neighbours are ("Batch-size independence").

One pool of initial conditions per kernel family is run once; prefixes, windows and a reversed prefix of the pool - at the
sizes where the packing of systems onto wavefronts and workgroups has its edges: 1, 2, 3, S - 1, S, S + 1, 2 S + 1 and 65
systems, S = the systems one wavefront (or workgroup) serves - are run on fresh integrators and compared with the pool
run's columns through np.array_equal: single steps with all Taylor coefficients, forward / backward / clamped steps,
propagate_until() with per-system final times (the systems of a wavefront finish at different moments; no batch here is
larger than what a launch keeps in flight, so no system is REFILLED into the lanes of a finished one - that path is
compared under the emulator, tests/test_emulated_kernels.py), propagate_grid(), and the event log of
the stepper which evaluates the event equations itself. Independence alone would pass if every size were wrong in the same
way: the pool run and the sizes 1, 2, 3 and S + 1 are also held to the oracle at the tolerances of the families' own
parity tests."""
import json
import os
import re

import numpy as np
import pytest

import heyoka_amd as hy
import heyoka_oracle as ho
from heyoka_amd import codegen_check, configs
from heyoka_amd import mixed_models as mm
from conftest import EPS

from test_gpu_parity import _random_system, nbody_row_classes, rel_err, row_rel_err

OC = hy.taylor_outcome
M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
HERE = os.path.dirname(os.path.abspath(__file__))
N_POOL = 131
WINDOW_START = 5  # (not a multiple of any S)


# ---- the kernel families ----
def _ring_state(n_bodies, n, seed=3):
    """Planets on perturbed circular orbits around a heavy first body with random phases (the systems of
    test_pair_kernels_with_17_to_32_pairs): the step sizes and step counts differ from system to system."""
    rng = np.random.RandomState(seed)
    st = np.zeros((6 * n_bodies, n))
    for b in range(1, n_bodies):
        r = 1.0 + 0.7 * b
        ph = rng.uniform(0, 2 * np.pi, n)
        v = 1.0 / np.sqrt(r)
        st[6 * b + 0], st[6 * b + 1], st[6 * b + 2] = r * np.cos(ph), r * np.sin(ph), 0.01 * rng.randn(n)
        st[6 * b + 3], st[6 * b + 4], st[6 * b + 5] = -v * np.sin(ph), v * np.cos(ph), 0.01 * rng.randn(n)
    return st


def _ring_masses(n_bodies):
    return [1.0] + [1e-3 * (i + 1) for i in range(n_bodies - 1)]


def _vars(m, *names):
    return [m.var(s) for s in names] if m is ho else [hy.make_vars(s, "dummy__")[0] for s in names]


def tan_system(m):
    x, y = _vars(m, "x", "y")
    return [(x, 0.3 * m.tan(y) - 0.4 * x), (y, -0.3 * m.tan(x) * m.cos(y) - 0.4 * y)]


def _centres():
    # (The system and the states of test_every_stepper_is_deterministic_run_to_run: one stream of random numbers.)
    rs = np.random.RandomState(11)
    masses, positions = list(rs.uniform(0.5, 1.5, 100) / 100.0), list(rs.uniform(-1.0, 1.0, 300))
    return masses, positions, rs


def _centres_state(n):
    rs = _centres()[2]
    return np.concatenate([rs.uniform(1.5, 2.0, (3, n)), rs.uniform(-0.3, 0.3, (3, n))])


def _np1body_state(n):
    full = configs.outer_ss_state(n, perturb=1e-3, seed=3).reshape(6, 6, n)
    return (full[1:] - full[:1]).reshape(30, n)


def _cr3bp_state(n):
    with open(os.path.join(HERE, "golden", "model_structure_pins.json")) as f:
        b = np.asarray(json.load(f)["cr3bp"]["init_state"], dtype=np.float64)[:, None]
    rng = np.random.RandomState(1)
    return np.ascontiguousarray(b + (np.abs(b) + 0.05) * 1e-3 * rng.uniform(-1, 1, (b.shape[0], n)))


def _random_pool(n):
    rs = np.random.RandomState(100 + 1008)
    return rs.uniform(-0.7, 0.7, (3, n)), rs.uniform(-0.5, 0.5, (2, n)), rs.uniform(0.0, 2.0, n)


def _outer_ss_events(m, log):
    """The event equations of 'outer_ss_event_equations_inside_the_stepper' (test_codegen_hazards.py): Saturn crossing
    y = 0, Jupiter overtaking Saturn in x, their distance passing 9 AU (non-terminal) and Jupiter crossing x = 3 (terminal;
    its callback keeps the system going - a stopping terminal event ends the propagation of the whole batch in the
    reference). Every callback logs (index of the system in its batch, event, time, sign)."""
    x1, y1, z1, x2, y2, z2 = _vars(m, "x_1", "y_1", "z_1", "x_2", "y_2", "z_2")
    d2 = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2) - 81.0

    def nt(k):
        return lambda ta, t, d, i: log.append((int(i), k, float(t), int(d), 0.0))

    def te(ta, d, i):
        # (The callback of a terminal event is not given the time: the system's time, which the step has just set to it.)
        hi, lo = (ta.time_hi, ta.time_lo) if m is ho else ta.dtime
        log.append((int(i), 3, float(hi[i]), int(d), float(lo[i])))
        return True

    return dict(nt_events=[m.nt_event(y2, nt(0)), m.nt_event(x1 - x2, nt(1)), m.nt_event(d2, nt(2))],
                t_events=[m.t_event(x1 - 3.0, te)])


_ONE_LANE_OFF = {"HEYOKA_AMD_ONE_LANE": "0"}
_PIPELINED = {"HEYOKA_AMD_ONE_LANE": "0", "HEYOKA_AMD_PAIR_SPLIT": "0"}


def _outer(**extra):
    d = dict(sys=lambda m: m.model.nbody(6, masses=M, Gconst=G) if m is hy else m.nbody(6, masses=M, Gconst=G),
             kw=dict(high_accuracy=True), okw=dict(high_accuracy=True), t_end=30.0,
             pool=lambda n: (configs.outer_ss_state(n, perturb=1e-3, seed=3), None, None))
    d.update(extra)
    return d


def _rings(nb, **extra):
    d = dict(sys=lambda m: m.model.nbody(nb, masses=_ring_masses(nb)) if m is hy else m.nbody(nb, masses=_ring_masses(nb)),
             kw=dict(high_accuracy=True), okw=dict(high_accuracy=True), t_end=8.0, pool=lambda n: (_ring_state(nb, n), None, None))
    d.update(extra)
    return d


def _plummer(nb, **extra):
    d = dict(sys=lambda m: m.model.nbody(nb) if m is hy else m.nbody(nb), t_end=0.02, prop_tol=1e7,
             pool=lambda n: (configs.plummer_nbody_state(nb, n, seed=3, jitter=1e-3), None, None))
    d.update(extra)
    return d


def _rnd(**extra):
    d = dict(sys=lambda m: _random_system(m, np.random.RandomState(1008), extended=True), pool=_random_pool, t_end=0.5,
             kw=dict(emitter="table"), floor_at_one=True)
    d.update(extra)
    return d


# name -> description of a family. want: substrings of hip_source_mode; t_end: propagate_until() goes to t0 + t_end * U(0.5,
# 1.5) (the horizons of test_every_stepper_is_deterministic_run_to_run and of the families' parity tests); prop_tol: the
# tolerance, in eps, of the states after the propagation in the family's own parity test (1e6 unless stated: 1e7 in
# test_models.py and _nbody_parity()); floor_at_one: states compared with rel_err() as in the family's parity test.
FAMILIES = {
    "v5": _outer(want=["mode v5", "lanes per system: 16"]),
    "v5_32_lanes": _rings(8, want=["mode v5", "lanes per system: 32"]),
    "v5_8_lanes_lds_jets": _rings(3, want=["mode v5", "lanes per system: 8", "jets in LDS"]),
    "v5_16_lanes_lds_jets": _rings(4, want=["mode v5", "lanes per system: 16", "jets in LDS"]),
    "v5_events": _outer(want=["mode v5", "inside the stepper", "4 event equation(s)"], events=True),
    "v3": _outer(env=_ONE_LANE_OFF, want=["mode v3", "lanes per system: 32"]),
    "v3_64_lanes": _rings(7, env=_ONE_LANE_OFF, want=["mode v3", "lanes per system: 64"]),
    "v2": _outer(env=_PIPELINED, want=["mode v2", "pipelined"]),
    "v2_aliased": dict(sys=lambda m: m.model.np1body(6, masses=M, Gconst=G) if m is hy else m.np1body(6, masses=M, Gconst=G),
                       want=["mode v2", "aliased"], t_end=30.0, prop_tol=1e7, pool=lambda n: (_np1body_state(n), None, None)),
    "multi_class": dict(sys=lambda m: mm.sine_lattice(m, 16), want=["classes of clusters"], t_end=2.0, prop_tol=1e7, mixed=True,
                        pool=lambda n: (mm.sine_lattice_state(16, n, seed=3), None, None)),
    "unrolled": dict(sys=tan_system, want=["unrolled", "lanes per system: 1,"], t_end=0.8, floor_at_one=True,
                     pool=lambda n: (np.random.RandomState(7).uniform(-0.6, 0.6, (2, n)), None, None)),
    "unrolled_two_waves": dict(sys=lambda m: m.model.nbody(2, masses=[1.0, 0.0]) if m is hy else m.nbody(2, masses=[1.0, 0.0]),
                               want=["unrolled", "two wavefronts per SIMD"], t_end=30.0, floor_at_one=True,
                               # (The orbits of test_two_body_stepwise_and_kepler_invariants, eccentricity up to 0.05, not
                               # the 1e-3 of the determinism test: the circular orbit is the singular point of the
                               # step-size selector - its order-p coefficients are cancellations - and at 1e-3 the
                               # oracle's own two orders of the operations, default and compact mode, disagree on h by
                               # up to 3.5e6 eps over this pool, more than the 1e6 eps of the parity tests; at 0.05 by
                               # 1.7e4 eps. Every other pool: at most 1.3e4 eps, most below 2 eps.)
                               pool=lambda n: (configs.two_body_state(n, perturb=0.05, seed=11), None, None)),
    "unrolled_register_jets": dict(sys=lambda m: m.model.cr3bp() if m is hy else m.cr3bp(), t_end=5.0, prop_tol=1e7,
                                   want=["unrolled", "register-resident state jets"], pool=lambda n: (_cr3bp_state(n), None, None)),
    "staged": _outer(kw=dict(high_accuracy=True, emitter="table"), want=["table mode (staged)"], t_end=5.0, spills=True),
    "table_hbm": _outer(kw=dict(high_accuracy=True, emitter="table"), env={"HEYOKA_AMD_TABLE_LDS": "0"}, want=["tape in HBM"], t_end=5.0),
    "staged_functions": _rnd(want=["table mode (staged)"], spills=True),
    "table_hbm_functions": _rnd(env={"HEYOKA_AMD_TABLE_LDS": "0"}, want=["tape in HBM"]),
    "block_centres": dict(sys=lambda m: m.model.fixed_centres(masses=_centres()[0], positions=_centres()[1]) if m is hy
                          else m.fixed_centres(masses=_centres()[0], positions=_centres()[1]),
                          want=["block mode", "100 clusters"], not_want="v2 cluster phase", t_end=0.5, prop_tol=1e7,
                          pool=lambda n: (_centres_state(n), None, None)),
    "block_v2": _plummer(12, want=["block mode", "v2 cluster phase", "66 clusters"]),
    "block_v2_nbody64": _plummer(64, want=["block mode", "v2 cluster phase", "2016 clusters"], n_pool=9, sizes=[1, 2, 3], n_oracle=3),
}

def systems_per_unit(mode):
    """S: the systems which one wavefront (cluster kernels, one-lane-per-system kernels) or one workgroup (a system on 64
    lanes or more: staged table stepper, lane-pair kernel at 64 lanes, block kernels) serves, from what the generator
    reports in hip_source_mode."""
    lanes = int(re.search(r"lanes per system: (\d+)", mode).group(1))
    return max(1, 64 // lanes)


def sizes_for(S, n_pool):
    out = []
    for n in (1, 2, 3, S - 1, S, S + 1, 2 * S + 1, 65):
        if 0 < n <= n_pool and n not in out:
            out.append(n)
    return out


class _env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _inputs(fam, n_pool):
    """Everything a system is given, as a function of its index in the pool."""
    st, pars, t0 = fam["pool"](n_pool)
    rs = np.random.RandomState(1)
    t0v = np.zeros(n_pool) if t0 is None else np.asarray(t0)
    idx = np.arange(n_pool)
    return dict(st=np.ascontiguousarray(st), pars=pars, t0=t0, tf=t0v + fam["t_end"] * rs.uniform(0.5, 1.5, n_pool),
                grid_span=0.25 * fam["t_end"] * (1.0 + 0.03 * (idx % 7)))


def run_subset(fam, inp, idx, step_limits=None):
    """The operations of the test on a fresh integrator which holds the systems idx of the pool, in that order. Returns
    (dict of recorded arrays - the last axis runs over the systems - , the integrator, event log by pool index)."""
    idx = np.asarray(idx)
    n = idx.size
    kw = dict(fam.get("kw", {}))
    log = []
    if inp["pars"] is not None:
        kw["pars"] = np.ascontiguousarray(inp["pars"][:, idx])
    if inp["t0"] is not None:
        kw["time"] = np.ascontiguousarray(inp["t0"][idx])
    if fam.get("events"):
        kw.update(_outer_ss_events(hy, log))
    with _env(fam.get("env")):
        ta = hy.taylor_adaptive_batch(fam["sys"](hy), np.ascontiguousarray(inp["st"][:, idx]), n, **kw)
    for w in fam["want"]:
        assert w in ta.hip_source_mode, (w, ta.hip_source_mode)
    assert fam.get("not_want", "\0") not in ta.hip_source_mode, ta.hip_source_mode
    rec = {}

    def snap(tag, tc=False):
        hi, lo = ta.dtime
        sr = ta.step_res
        rec[tag + " state"], rec[tag + " time hi"], rec[tag + " time lo"] = np.asarray(ta.state).copy(), hi.copy(), lo.copy()
        rec[tag + " outcome"] = np.array([int(o) for o, _ in sr], dtype=np.int64)
        rec[tag + " h"] = np.array([h for _, h in sr])
        if tc:
            rec[tag + " Taylor coefficients"] = np.asarray(ta.tc).copy()

    # 1. One step with all Taylor coefficients.
    ta.step(write_tc=True)
    snap("step 1", tc=True)
    # 2. Forward, backward, and forward with a limit which clamps the odd systems of the pool to half their first step.
    ta.step()
    snap("step 2")
    ta.step_backward()
    snap("step 3 (backward)")
    h1 = rec["step 1 h"] if step_limits is None else step_limits[idx]
    lim = np.where(idx % 2 == 1, 0.5, 1e3) * np.abs(h1)
    ta.step(max_delta_t=lim)
    snap("step 4 (limited)")
    # 3. Propagation to per-system final times.
    ta.propagate_until(inp["tf"][idx])
    oc, mn, mx, ns = ta.propagate_res_arrays()
    hi, lo = ta.dtime
    rec.update({"propagate_until state": np.asarray(ta.state).copy(), "propagate_until time hi": hi.copy(), "propagate_until time lo": lo.copy(),
                "propagate_until outcome": np.asarray(oc, dtype=np.int64).copy(), "propagate_until min |h|": np.asarray(mn).copy(),
                "propagate_until max |h|": np.asarray(mx).copy(), "propagate_until steps": np.asarray(ns).astype(np.int64)})
    # 4. A grid of 5 points per system, no callback.
    grid = hi[None, :] + np.linspace(0.0, 1.0, 5)[:, None] * inp["grid_span"][idx][None, :]
    _, out = ta.propagate_grid(grid)
    oc, mn, mx, ns = ta.propagate_res_arrays()
    rec.update({"propagate_grid samples": np.asarray(out).copy(), "propagate_grid state": np.asarray(ta.state).copy(),
                "propagate_grid time hi": ta.dtime[0].copy(), "propagate_grid outcome": np.asarray(oc, dtype=np.int64).copy(),
                "propagate_grid steps": np.asarray(ns).astype(np.int64)})
    # 5. The events of every system in the order in which its callbacks ran (sorted() is stable).
    ev = sorted([(int(idx[i]), k, t, d, lo) for i, k, t, d, lo in log], key=lambda e: e[0])
    return rec, ta, ev


def assert_same_as_pool(label, rec, pool_rec, idx, ev=None, pool_ev=None):
    for key, val in rec.items():
        want = pool_rec[key][..., idx]
        assert not np.isnan(val).any(), (label, key)
        if not np.array_equal(val, want):
            bad = np.argwhere(val != want)
            first = tuple(bad[0])
            raise AssertionError("%s: '%s' differs from the pool run in %d entries of %d; first at %s (system %d of the batch, pool index "
                                 "%d): %r here, %r in the pool run" % (label, key, len(bad), val.size, first, first[-1], idx[first[-1]],
                                                                       val[first], want[first]))
    if ev is not None:
        sel = set(int(i) for i in idx)
        assert ev == [e for e in pool_ev if e[0] in sel], label


# ---- against the oracle ----
def run_oracle(fam, inp, n, lims):
    """The same operations 1 .. 3 on the oracle for the first n systems of the pool."""
    idx = np.arange(n)
    kw = dict(fam.get("okw", {}))
    log = []
    if inp["pars"] is not None:
        kw["pars"] = np.ascontiguousarray(inp["pars"][:, idx])
    if inp["t0"] is not None:
        kw["time"] = np.ascontiguousarray(inp["t0"][idx])
    st = np.ascontiguousarray(inp["st"][:, idx])
    if fam.get("events"):
        ora = ho.OracleEventIntegrator(fam["sys"](ho), st, n, **_outer_ss_events(ho, log), **kw)
    else:
        ora = ho.OracleIntegrator(fam["sys"](ho), st, n, **kw)
    dim = st.shape[0]
    o = {}
    ora.step(wtc=True)
    o["step 1 h"] = np.array([h for _, h in ora.step_res])
    o["step 1 outcome"] = np.array([int(c) for c, _ in ora.step_res], dtype=np.int64)
    o["step 1 state"] = ora.state.reshape(dim, n).copy()
    o["step 1 Taylor coefficients"] = ora.tc.reshape(dim, ora.order + 1, n).copy()
    ora.step()
    ora.step(backward=True)
    ora.step(max_delta_ts=lims[idx])
    ora.propagate_until(inp["tf"][idx])
    o["propagate_until state"] = ora.state.reshape(dim, n).copy()
    o["propagate_until time hi"] = ora.time_hi.copy()
    o["propagate_until outcome"] = np.array([int(r[0]) for r in ora.prop_res], dtype=np.int64)
    o["propagate_until steps"] = np.array([int(r[3]) for r in ora.prop_res], dtype=np.int64)
    o["events"] = sorted(log, key=lambda e: e[0])
    return o


def assert_close_to_oracle(label, fam, rec, ev, o, idx):
    """rec: a run of the systems idx of the pool; o: the oracle's run of the pool. The tolerances of the families' parity
    tests (tests/test_gpu_parity.py, tests/test_models.py): h 1e6 eps, Taylor coefficients 1e6 eps of the row maximum, states
    1e5 eps after the step and prop_tol (1e6 or 1e7) eps after the propagation - rows scaled by their maximum over the pool,
    or with rel_err() where the family's own test does -, step counts within 1, outcomes equal. The rows of a small batch are
    scaled like those of the pool: the columns of the oracle's pool run which the batch does not hold stand in for
    themselves."""
    idx = np.asarray(idx)

    def embed(key):
        full = o[key].copy()
        full[..., idx] = rec[key]
        return full

    h_o = o["step 1 h"][idx]
    e_h = float(np.max(np.abs(rec["step 1 h"] - h_o) / np.abs(h_o))) / EPS
    assert np.array_equal(rec["step 1 outcome"], o["step 1 outcome"][idx]), label
    tc_o = o["step 1 Taylor coefficients"]
    scale = np.max(np.abs(tc_o), axis=2, keepdims=True) + 1e-300
    e_tc = float(np.max(np.abs(embed("step 1 Taylor coefficients") - tc_o) / scale)) / EPS
    err = rel_err if fam.get("floor_at_one") else row_rel_err
    e_s1 = float(err(embed("step 1 state"), o["step 1 state"])) / EPS
    e_pr = float(err(embed("propagate_until state"), o["propagate_until state"])) / EPS
    dn = int(np.max(np.abs(rec["propagate_until steps"] - o["propagate_until steps"][idx])))
    print("[%s vs oracle, eps] h %.3g, Taylor coefficients %.3g, state after the step %.3g, after the propagation %.3g (%d .. %d "
          "steps, largest difference %d)" % (label, e_h, e_tc, e_s1, e_pr, o["propagate_until steps"][idx].min(),
                                             o["propagate_until steps"][idx].max(), dn))
    dim = o["step 1 state"].shape[0]
    if dim % 6 == 0 and dim >= 12 and not fam.get("floor_at_one"):
        nbody_row_classes(embed("step 1 state"), o["step 1 state"], label + ", step")
        nbody_row_classes(embed("propagate_until state"), o["propagate_until state"], label + ", propagation")
    if fam.get("mixed"):
        # (test_mixed_models_step_and_propagate_vs_oracle: h and the state after the step only on the lanes on which the two
        # flavours of the oracle agree on h; that test finds all but 4 of 48 such.)
        well = o["well"][idx]
        assert np.count_nonzero(~o["well"]) <= o["well"].size // 12
        e_h = float(np.max((np.abs(rec["step 1 h"] - h_o) / np.abs(h_o))[well], initial=0.0)) / EPS
        keep = np.ones(o["well"].size, dtype=bool)
        keep[idx[~well]] = False
        e_s1 = float(err(embed("step 1 state")[:, keep], o["step 1 state"][:, keep])) / EPS
    assert e_h <= 1e6 and e_tc <= 1e6 and e_s1 <= 1e5 and e_pr <= fam.get("prop_tol", 1e6), label
    assert np.array_equal(rec["propagate_until outcome"], o["propagate_until outcome"][idx]), label
    assert np.all(np.abs(rec["propagate_until time hi"] - o["propagate_until time hi"][idx])
                  <= 2.0 * np.spacing(np.abs(o["propagate_until time hi"][idx]))), label
    assert dn <= 1, label
    if fam.get("events"):
        sel = set(int(i) for i in idx)
        # (The oracle ran operations 1 - 3: the events of the grid are not in its log.)
        ev_o = [e for e in o["events"] if e[0] in sel]
        per_sys = {}
        for e in ev_o:
            per_sys[e[0]] = per_sys.get(e[0], 0) + 1
        ev_g, seen = [], {}
        for e in ev:
            seen[e[0]] = seen.get(e[0], 0) + 1
            if seen[e[0]] <= per_sys.get(e[0], 0):
                ev_g.append(e)
        assert [(e[0], e[1], e[3]) for e in ev_g] == [(e[0], e[1], e[3]) for e in ev_o], label
        assert len(ev_o) >= len(sel)
        assert max(abs(a[2] - b[2]) for a, b in zip(ev_g, ev_o)) <= 1e-10, label


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_results_do_not_depend_on_batch_size_position_or_neighbours(family):
    """See the module docstring. Prints the family's S as derived from hip_source_mode, its sizes and the measured errors
    against the oracle."""
    fam = FAMILIES[family]
    n_pool = fam.get("n_pool", N_POOL)
    inp = _inputs(fam, n_pool)
    pool_idx = np.arange(n_pool)
    pool, ta, pool_ev = run_subset(fam, inp, pool_idx)
    lims_by_pool_index = np.abs(pool["step 1 h"])
    mode, src = ta.hip_source_mode, ta.hip_source
    S = systems_per_unit(mode)
    sizes = fam.get("sizes") or sizes_for(S, n_pool)
    print("\n[%s] %s\n[%s] S = %d system(s) per %s, pool of %d, sizes %s" % (family, mode.split(";")[0], family, S,
                                                                            "wavefront" if S > 1 else "workgroup", n_pool, sizes))
    if fam.get("spills"):
        res = codegen_check.kernel_resources(ta.code_object)
        print("[%s] spilled VGPRs: %d (known, tracked separately)" % (family, res["vgpr_spill"]))
    assert not any(np.isnan(v).any() for v in pool.values())
    assert np.all(pool["propagate_until outcome"] == int(OC.time_limit))
    # (The last step is clamped to the high part of the remaining time and the new time is a double-length sum: the pair
    # (hi, lo) ends on the final time, hi alone within an ulp of it - in the reference and the oracle as well.)
    t_err = np.abs((pool["propagate_until time hi"] - inp["tf"]) + pool["propagate_until time lo"])
    assert np.all(t_err <= 4.0 * EPS * np.maximum(1.0, np.abs(inp["tf"])))
    assert np.unique(pool["propagate_until steps"]).size > 1  # (the systems finish at different moments)
    clamped = pool["step 4 (limited) outcome"] == int(OC.time_limit)
    assert 0.3 * n_pool <= np.count_nonzero(clamped) <= 0.7 * n_pool  # (the limit clamps about half of the systems)
    del ta

    reversed_size = 3 if S + 1 not in sizes else S + 1
    runs = {}
    for n in sizes:
        a = WINDOW_START if WINDOW_START + n <= n_pool else n_pool - n
        subsets = [("prefix", np.arange(n))]
        if a > 0:
            subsets.append(("window %d:%d" % (a, a + n), np.arange(a, a + n)))
        if n == reversed_size:
            subsets.append(("reversed prefix", np.arange(n)[::-1].copy()))
        for what, idx in subsets:
            label = "%s, n = %d, %s" % (family, n, what)
            rec, tb, ev = run_subset(fam, inp, idx, step_limits=lims_by_pool_index)
            assert tb.hip_source == src, label + ": the generated source depends on the batch size"
            del tb
            assert_same_as_pool(label, rec, pool, idx, ev if fam.get("events") else None, pool_ev)
            if what == "prefix":
                runs[n] = (rec, ev)

    n_or = fam.get("n_oracle", n_pool)
    o = run_oracle(fam, inp, n_or, np.where(pool_idx % 2 == 1, 0.5, 1e3) * lims_by_pool_index)
    if fam.get("mixed"):
        oc_ = ho.OracleIntegrator(fam["sys"](ho), inp["st"], n_pool, compact_mode=True)
        oc_.step()
        h_c = np.array([h for _, h in oc_.step_res])
        o["well"] = np.abs(h_c - o["step 1 h"]) / np.abs(o["step 1 h"]) <= 1e3 * EPS
    sub = np.arange(n_or)
    assert_close_to_oracle("%s, pool" % family, fam, {k: v[..., sub] for k, v in pool.items()}, pool_ev, o, sub)
    for n in [m for m in sorted({1, 2, 3, S + 1}) if m in runs and m <= n_or]:
        assert_close_to_oracle("%s, n = %d" % (family, n), fam, runs[n][0], runs[n][1], o, np.arange(n))
