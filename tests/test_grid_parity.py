"""propagate_grid() and the dense output against the grid oracle (oracle/heyoka_oracle.py: OracleIntegrator.propagate_grid,
the reference's propagate_grid_impl() restated line by line) and against mpmath.

Every grid path of the library - the multi-step launches of the one-lane-per-pair stepper, its single-step sweeps with a
step limit or a callback, the other cluster kernels, the straight-line, table and block steppers, the stepper with events,
the lock-step semantics and the device-buffer variant - runs the same inputs as the oracle, lane by lane: outcomes and the
NaN pattern of the samples exactly, step counts exactly (or the README's +-1 on at most 1 % of the lanes), samples and final
states with a per-row scale. The dense-output arithmetic itself (the grid's post-step kernel, update_d_output()) is held to
the a-priori error bound of its algorithm around the exact value of the integrator's own Taylor polynomial, evaluated in
mpmath at the exact offset."""
import numpy as np
import pytest

import heyoka_amd as hy
import heyoka_oracle as ho
from heyoka_amd import configs
from conftest import EPS

pytestmark = pytest.mark.gpu

OC = hy.taylor_outcome
M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G


def row_rel_err(a, b):
    """Per-row scale (rows = grid point x state variable, columns = lanes), as test_gpu_parity.row_rel_err(); NaN entries
    (unreached grid points, equal in both) count as zero."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = np.nan_to_num(a.reshape(-1, b.shape[-1])), np.nan_to_num(b.reshape(-1, b.shape[-1]))
    scale = np.max(np.abs(b), axis=1) + 1e-300
    return float(np.max(np.max(np.abs(a - b), axis=1) / scale))


def check_against_oracle(label, ta, out, ora, out_o, tol=1e6, strict_steps=False):
    """Outcomes exact, NaN pattern exact, step counts exact (+-1 on at most 1 % of the lanes unless strict_steps), samples and
    final states per-row within tol eps. Prints the measured errors."""
    n = ta.batch_size
    pr, pr_o = ta.propagate_res, ora.prop_res
    assert [int(r[0]) for r in pr] == [int(r[0]) for r in pr_o], label
    assert np.array_equal(np.isnan(out), np.isnan(out_o)), label
    dn = np.abs(np.array([int(r[3]) for r in pr]) - np.array([int(r[3]) for r in pr_o]))
    if strict_steps:
        assert np.all(dn == 0), (label, dn)
    else:
        assert np.all(dn <= 1) and np.count_nonzero(dn) <= n // 100, (label, dn)
    e_out = row_rel_err(out, out_o) / EPS
    e_st = row_rel_err(ta.state, ora.state.reshape(-1, n)) / EPS
    print("[grid vs oracle] %-28s samples %.3g eps, final states %.3g eps, steps %d..%d, lanes with a step-count "
          "difference %d" % (label, e_out, e_st, min(r[3] for r in pr_o), max(r[3] for r in pr_o), np.count_nonzero(dn)))
    dim = out.shape[1]
    if dim % 6 == 0 and dim >= 12:
        # Per row class of an N-body state (body-major rows x, y, z, vx, vy, vz), the samples' rows over grid points x lanes.
        a = np.nan_to_num(np.transpose(out, (1, 0, 2)).reshape(dim, -1))
        b = np.nan_to_num(np.transpose(out_o, (1, 0, 2)).reshape(dim, -1))
        rows = (np.max(np.abs(a - b), axis=1) / (np.max(np.abs(b), axis=1) + 1e-300) / EPS).reshape(dim // 6, 6)
        print("[grid vs oracle] %-28s per row class, eps: first body %.3g, others x, y, vx, vy %.3g, others z, vz %.3g"
              % (label, np.max(rows[0]), np.max(rows[1:][:, [0, 1, 3, 4]]), np.max(rows[1:][:, [2, 5]])))
    assert e_out <= tol and e_st <= tol, label


def outer_ss(n, seed, **kw):
    st = configs.outer_ss_state(n, perturb=1e-6, seed=seed)
    return hy.model.nbody(6, masses=M, Gconst=G), ho.nbody(6, masses=M, Gconst=G), st


def lane_grid(n, t_end, n_pts, backward=False):
    """Per-lane grids: the same number of points, a spacing which differs from lane to lane by up to 3 %."""
    g = np.outer(np.linspace(0.0, t_end, n_pts), 1.0 + 0.03 * np.arange(n) / max(n - 1, 1))
    return -g if backward else g


def pendulum(m):
    if m is ho:
        x, v = ho.var("x"), ho.var("v")
    else:
        x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -9.8 * m.sin(x))]


def _mode(ta, want):
    assert want in ta.hip_source_mode, ta.hip_source_mode


class _log_capture:
    def __enter__(self):
        self.msgs = []
        hy.set_log_callback(lambda lvl, m: self.msgs.append(m))
        hy.set_logger_level_debug()
        return self

    def __exit__(self, *exc):
        hy.set_logger_level("warn")
        hy.set_log_callback(None)

    def grid_lines(self):
        return [m for m in self.msgs if "propagate_grid() loop:" in m]


# ---- 1. lane-by-lane parity of every grid path ----
def test_v5_multi_step_grid_vs_oracle_one_launch_per_interval():
    """The headline path: no callback, no events, no step limit - one launch per grid interval (the debug line of the grid
    loop says which loop ran and how many stepper launches it took). 67 systems (not a multiple of the four systems of a
    wavefront), per-lane grids forward and then backward to the start, and max_delta_t below the natural step."""
    n = 67
    sys_g, sys_o, st = outer_ss(n, 41)
    grid = lane_grid(n, 30.0, 13)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    _mode(ta, "v5")
    with _log_capture() as lc:
        _, out = ta.propagate_grid(grid)
    lines = lc.grid_lines()
    assert len(lines) == 1 and "multi-step launches" in lines[0] and "12 stepper launches for 12 grid intervals" in lines[0], lines
    ora = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, out_o = ora.propagate_grid(grid)
    check_against_oracle("v5 multi-step", ta, out, ora, out_o)
    # Backward over the same grid, back to the start.
    gb = grid[::-1].copy()
    _, outb = ta.propagate_grid(gb)
    _, outb_o = ora.propagate_grid(gb)
    check_against_oracle("v5 multi-step backward", ta, outb, ora, outb_o)
    # max_delta_t below the natural step (about 0.42 years).
    tb = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    _, out2 = tb.propagate_grid(grid[:5], max_delta_t=0.1)
    orb = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, out2_o = orb.propagate_grid(grid[:5], max_delta_t=0.1)
    check_against_oracle("v5 multi-step max_delta_t", tb, out2, orb, out2_o, strict_steps=True)


def test_v5_single_step_sweeps_step_limit_and_callback_vs_oracle():
    """The one-lane-per-pair stepper in single-step sweeps: max_steps ending between two grid points (step_limit, NaN rows
    beyond), and a step callback (a sweep per step, the coefficients of every step; one call per sweep on both sides)."""
    n = 67
    sys_g, sys_o, st = outer_ss(n, 42)
    grid = lane_grid(n, 10.0, 9)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    _mode(ta, "v5")
    with _log_capture() as lc:
        _, out = ta.propagate_grid(grid, max_steps=11)
    assert "single-step sweeps" in lc.grid_lines()[0]
    ora = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, out_o = ora.propagate_grid(grid, max_steps=11)
    assert all(r[0] == OC.step_limit for r in ta.propagate_res)
    assert np.isnan(out_o[-1]).all() and not np.isnan(out_o[3]).any()
    check_against_oracle("v5 max_steps", ta, out, ora, out_o, strict_steps=True)
    calls, calls_o = [], []
    tb = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    _, outc = tb.propagate_grid(grid, callback=lambda t: calls.append(1) or True)
    orb = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, outc_o = orb.propagate_grid(grid, callback=lambda t: calls_o.append(1) or True)
    assert len(calls) == len(calls_o)
    check_against_oracle("v5 callback", tb, outc, orb, outc_o)


@pytest.mark.parametrize("kernel", ["v3", "v2"])
def test_other_cluster_kernels_grid_vs_oracle(kernel, monkeypatch):
    """The lane-pair kernel v3 and the pipelined v2: 5 systems, backward per-lane grids with max_delta_t."""
    monkeypatch.setenv("HEYOKA_AMD_ONE_LANE", "0")
    if kernel == "v2":
        monkeypatch.setenv("HEYOKA_AMD_PAIR_SPLIT", "0")
    n = 5
    sys_g, sys_o, st = outer_ss(n, 43)
    grid = lane_grid(n, 12.0, 7, backward=True)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    _mode(ta, kernel)
    _, out = ta.propagate_grid(grid, max_delta_t=1.5)
    ora = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, out_o = ora.propagate_grid(grid, max_delta_t=1.5)
    check_against_oracle(kernel, ta, out, ora, out_o)


def test_unrolled_steppers_grid_vs_oracle():
    """The straight-line stepper: two-body with the re-derived velocities (300 systems, more than the 256 threads of the
    post-step kernel's workgroup), and a single pendulum with several grid points inside one step, a grid point exactly at
    the end of the first step, and a start time of about 1e4 with a nonzero low part."""
    n = 300
    st = configs.two_body_state(n, perturb=1e-3, seed=44)
    ta = hy.taylor_adaptive_batch(hy.model.nbody(2, masses=[1.0, 0.0]), st, n)
    _mode(ta, "two wavefronts per SIMD")
    grid = lane_grid(n, 8.0, 11)
    _, out = ta.propagate_grid(grid)
    ora = ho.OracleIntegrator(ho.nbody(2, masses=[1.0, 0.0]), st, n)
    _, out_o = ora.propagate_grid(grid)
    check_against_oracle("unrolled two-body", ta, out, ora, out_o)

    st1 = np.array([[0.05], [0.025]])
    probe = ho.OracleIntegrator(pendulum(ho), st1, 1)
    probe.step()
    h1 = probe.last_h[0]
    grid1 = np.concatenate([np.linspace(0.0, h1, 6), h1 + np.linspace(0.0, 1.0, 7)[1:]])
    tp = hy.taylor_adaptive_batch(pendulum(hy), st1, 1)
    _mode(tp, "unrolled")
    _, outp = tp.propagate_grid(grid1)
    orp = ho.OracleIntegrator(pendulum(ho), st1, 1)
    _, outp_o = orp.propagate_grid(grid1)
    check_against_oracle("unrolled pendulum", tp, outp, orp, outp_o, strict_steps=True)
    # From t ~ 1e4 with a nonzero low part (three free steps), forward.
    tq = hy.taylor_adaptive_batch(pendulum(hy), st1, 1, time=1e4)
    orq = ho.OracleIntegrator(pendulum(ho), st1, 1, time=1e4)
    for _ in range(3):
        tq.step()
        orq.step()
    thi, tlo = tq.dtime
    assert thi[0] == orq.time_hi[0] and tlo[0] == orq.time_lo[0] and tlo[0] != 0.0
    gq = thi[0] + np.linspace(0.0, 2.0, 9)
    _, outq = tq.propagate_grid(gq)
    _, outq_o = orq.propagate_grid(gq)
    check_against_oracle("unrolled pendulum t ~ 1e4", tq, outq, orq, outq_o, strict_steps=True)


@pytest.mark.parametrize("variant", ["staged", "table_hbm"])
def test_table_steppers_grid_vs_oracle(variant, monkeypatch):
    """The table stepper in both variants (tape in LDS / in HBM) on the outer Solar System, 67 systems."""
    if variant == "table_hbm":
        monkeypatch.setenv("HEYOKA_AMD_TABLE_LDS", "0")
    n = 67
    sys_g, sys_o, st = outer_ss(n, 45)
    grid = lane_grid(n, 6.0, 7)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True, emitter="table")
    _mode(ta, {"staged": "staged", "table_hbm": "tape in HBM"}[variant])
    _, out = ta.propagate_grid(grid)
    ora = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, out_o = ora.propagate_grid(grid)
    check_against_oracle(variant, ta, out, ora, out_o)


def test_block_stepper_grid_vs_oracle():
    """Block mode: model::nbody(12) with distinct masses, 5 systems."""
    n, nb = 5, 12
    masses = list(1.0 / (1.0 + np.arange(nb)) ** 2 * nb / 4.0)
    st = configs.plummer_nbody_state(nb, n, seed=46, jitter=1e-6)
    ta = hy.taylor_adaptive_batch(hy.model.nbody(nb, masses=masses), st, n)
    _mode(ta, "block")
    grid = lane_grid(n, 0.02, 5)
    _, out = ta.propagate_grid(grid)
    ora = ho.OracleIntegrator(ho.nbody(nb, masses=masses), st, n)
    _, out_o = ora.propagate_grid(grid)
    check_against_oracle("block nbody(12)", ta, out, ora, out_o, tol=1e7)


def test_stepper_with_events_grid_vs_oracle():
    """The stepper with events (a non-terminal event: the event equations inside the one-lane-per-pair stepper) against
    OracleEventIntegrator: the samples, and the events in the same order at the same times."""
    n = 5
    sys_g, sys_o, st = outer_ss(n, 47)
    log_g, log_o = [], []
    x1, x2 = hy.make_vars("x_1", "x_2")
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True,
                                  nt_events=[hy.nt_event(x1 - x2, lambda t, tm, d, i: log_g.append((i, tm)))])
    _mode(ta, "inside the stepper")
    ora = ho.OracleEventIntegrator(sys_o, st, n, high_accuracy=True,
                                   nt_events=[ho.nt_event(ho.var("x_1") - ho.var("x_2"), lambda t, tm, d, i: log_o.append((i, tm)))])
    grid = lane_grid(n, 15.0, 7)
    _, out = ta.propagate_grid(grid)
    _, out_o = ora.propagate_grid(grid)
    check_against_oracle("events", ta, out, ora, out_o)
    assert [i for i, _ in sorted(log_g)] == [i for i, _ in sorted(log_o)] and len(log_o) > 0
    assert np.max(np.abs(np.array([t for _, t in sorted(log_g)]) - np.array([t for _, t in sorted(log_o)]))) <= 1e-9


def test_lockstep_semantics_and_device_buffer_grid_vs_oracle():
    """batch_semantics="lockstep" (single-step sweeps only) and propagate_grid_device() (samples written to a device
    buffer, multi-step launches) on the same inputs."""
    import torch

    n = 67
    sys_g, sys_o, st = outer_ss(n, 48)
    grid = lane_grid(n, 10.0, 6)
    ora = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    _, out_o = ora.propagate_grid(grid)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True, batch_semantics="lockstep")
    _mode(ta, "v5")
    with _log_capture() as lc:
        _, out = ta.propagate_grid(grid)
    assert "single-step sweeps" in lc.grid_lines()[0]
    check_against_oracle("lockstep", ta, out, ora, out_o)
    tb = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    d_out = torch.empty((grid.shape[0], 36, n), dtype=torch.float64, device="cuda")
    tb.propagate_grid_device(grid, d_out.data_ptr())
    torch.cuda.synchronize()
    check_against_oracle("propagate_grid_device", tb, d_out.cpu().numpy(), ora, out_o)


# ---- 4.1 a lane which goes non-finite between two grid points ----
def _collision_state(n, d=2.25):
    """Outer Solar Systems; in lane 1 Jupiter falls radially onto the Sun from d AU: non-finite at t = 0.597 for d = 2.25
    (the oracle's numbers, tests/test_oracle_golden.py)."""
    st = configs.outer_ss_state(n, perturb=1e-6, seed=3).reshape(36, n).copy()
    st[6:9, 1] = st[0:3, 1] + np.array([d, 0.0, 0.0])
    st[9:12, 1] = st[3:6, 1]
    return st


def _check_lockstep_stop(label, ta, out, ora, out_o, nf_lane=1):
    """A grid stopped by a lane which went non-finite, against the oracle's lock-step loop: outcomes, step counts and the NaN
    pattern of the samples exactly; the samples every run reached, and the healthy lanes' states and times, within 1e6 eps
    (per row) / 1e-12. Returns the number of sweeps."""
    n = ta.batch_size
    pr, pr_o = ta.propagate_res, ora.prop_res
    ok = np.arange(n) != nf_lane
    assert pr[nf_lane][0] == OC.err_nf_state, label
    assert [int(r[0]) for r in pr] == [int(r[0]) for r in pr_o], label
    ns, ns_o = np.array([int(r[3]) for r in pr]), np.array([int(r[3]) for r in pr_o])
    print("[non-finite stop] %s: steps of the healthy lanes %s (oracle %s), of the diverging lane %d (oracle %d)"
          % (label, sorted(set(ns[ok].tolist())), sorted(set(ns_o[ok].tolist())), ns[nf_lane], ns_o[nf_lane]))
    assert np.array_equal(ns, ns_o), label
    assert np.array_equal(np.isnan(out), np.isnan(out_o)), label
    assert row_rel_err(out, out_o) <= 1e6 * EPS, label
    assert row_rel_err(ta.state[:, ok], ora.state.reshape(-1, n)[:, ok]) <= 1e6 * EPS, label
    assert np.allclose(np.asarray(ta.time)[ok], ora.time_hi[ok], rtol=1e-12, atol=0.0), label
    return int(ns_o[0])


@pytest.mark.parametrize("semantics", [None, "per_lane"])
def test_a_nonfinite_lane_between_grid_points_stops_the_batch_after_that_sweep(semantics):
    """Reference semantics (the default): a lane which goes non-finite stops the whole batch after that sweep - also on the
    one-lane-per-pair stepper, whose grid is rolled back to its start and redone in single-step sweeps. Outcomes, step
    counts, NaN pattern, times and samples are the oracle's. batch_semantics="per_lane" keeps the asynchronous behaviour:
    the healthy lanes finish their current grid interval, and the non-finite lane's counters include the steps of its last
    launch. (max_delta_t = 0.01: every lane has taken the same number of steps at every grid point.)"""
    n = 67
    st = _collision_state(n)
    grid = np.linspace(0.0, 4.0, 9)
    sys_g = hy.model.nbody(6, masses=M, Gconst=G)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True, batch_semantics=semantics)
    _mode(ta, "v5")
    with _log_capture() as lc:
        _, out = ta.propagate_grid(grid, max_delta_t=0.01)
    print("[grid loop] %s" % lc.grid_lines())
    ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True)
    pr_o, out_o = ora.propagate_grid(grid, max_delta_t=0.01)
    pr = ta.propagate_res
    ok = np.array([i != 1 for i in range(n)])
    assert pr[1][0] == OC.err_nf_state and pr_o[1][0] == ho.OC_ERR_NF_STATE
    ns_o = np.array([r[3] for r in pr_o])
    ns = np.array([int(r[3]) for r in pr])
    if semantics is None:
        assert "rolled back to the start of the grid" in lc.grid_lines()[0]
        sweeps = _check_lockstep_stop("max_delta_t 0.01", ta, out, ora, out_o)
        assert np.isnan(out[:, :, ok][grid > 0.01 * sweeps + 1e-9]).all()
    else:
        # Per lane: every healthy lane runs on to the first step which reaches the end of the grid interval in which the
        # diverging lane stopped, and samples that grid point.
        assert "rolled back" not in lc.grid_lines()[0]
        t_ok = np.asarray(ta.time)[ok]
        k = 2  # (the diverging lane stops at t = 0.597, inside [grid[1], grid[2]])
        assert np.all(t_ok >= grid[k]) and np.all(t_ok < grid[k] + 0.0101), t_ok
        assert not np.isnan(out[: k + 1][:, :, ok]).any() and np.isnan(out[k + 1 :][:, :, ok]).all()
        assert 0.01 * ns_o[0] > grid[k]  # (the reference's lock-step batch stops later, at the diverging lane's sweep)
        # The non-finite lane: its steps before the non-finite one, all of them (its own propagation: the oracle's count).
        assert ns[1] == ns_o[1]
        assert np.isfinite(pr[1][1]) and pr[1][2] > 0.0


@pytest.mark.parametrize("semantics", [None, "lockstep"])
def test_a_nonfinite_lane_stops_lanes_with_different_step_counts_at_the_same_sweep(semantics):
    """Without max_delta_t the lanes reach a grid point after different numbers of steps (at t = 0.5 the healthy lanes have
    taken 2, the falling one 11): the lock-step batch stops every healthy lane after the sweep in which the diverging lane
    goes non-finite (sweep 203 of the oracle, t = 149), not after the same number of steps past the last grid point - the
    one-lane-per-pair stepper's multi-step launches are undone back to the start of the grid for that. And that sweep
    leaves no samples: the reference takes the samples of a step at the top of its NEXT iteration, which never comes (the
    healthy lanes cross t = 148.5 and 149 in their last step: NaN there)."""
    n = 5
    st = _collision_state(n)
    grid = np.linspace(0.0, 300.0, 601)
    ta = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True, batch_semantics=semantics)
    _mode(ta, "v5")
    with _log_capture() as lc:
        _, out = ta.propagate_grid(grid)
    print("[grid loop] %s" % lc.grid_lines())
    if semantics is None:
        assert "rolled back to the start of the grid" in lc.grid_lines()[0]
    else:
        assert "single-step sweeps" in lc.grid_lines()[0]
    ora = ho.OracleIntegrator(ho.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True)
    _, out_o = ora.propagate_grid(grid)
    sweeps = _check_lockstep_stop("no max_delta_t", ta, out, ora, out_o)
    # (The healthy lanes stop mid-grid, about 150 years in: the grid points beyond are NaN.)
    assert 100.0 < ora.time_hi[0] < 200.0 and np.isnan(out[-1]).all() and sweeps > 100


def test_a_lane_nonfinite_from_the_start_of_the_grid():
    """The simple case: a NaN in the state of one lane. The initial propagate_until() of the grid stops: outcomes kept,
    counters reset, every sample NaN - the oracle's result."""
    n = 5
    sys_g, sys_o, st = outer_ss(n, 49)
    st = st.reshape(36, n).copy()
    st[7, 2] = np.nan
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True)
    _, out = ta.propagate_grid(np.linspace(0.0, 3.0, 4))
    ora = ho.OracleIntegrator(sys_o, st, n, high_accuracy=True)
    pr_o, out_o = ora.propagate_grid(np.linspace(0.0, 3.0, 4))
    assert [int(r[0]) for r in ta.propagate_res] == [int(r[0]) for r in pr_o]
    assert [(r[1], r[2], int(r[3])) for r in ta.propagate_res] == [r[1:] for r in pr_o]
    assert np.isnan(out).all() and np.isnan(out_o).all()


# ---- 4.2 tc_stale ----
def test_interrupted_grid_with_coefficients_on_demand_refuses_the_taylor_coefficients():
    """After a grid interrupted by a non-finite lane, with the coefficients stored on demand (only the steps which reach a
    grid point store theirs), the lanes which did not reach a grid point in the last sweep hold the coefficients of an
    OLDER step: get_tc() / update_d_output() refuse them. A step without coefficients does not change that; a step which
    stores them all does."""
    n = 67
    st = _collision_state(n)
    ta = hy.taylor_adaptive_batch(hy.model.nbody(6, masses=M, Gconst=G), st, n, high_accuracy=True)
    ta.propagate_grid(np.linspace(0.0, 4.0, 9), max_delta_t=0.01)
    assert ta.propagate_res[1][0] == OC.err_nf_state
    msg = "The Taylor coefficients of the last step are not available"
    with pytest.raises(RuntimeError, match=msg):
        ta.tc
    with pytest.raises(RuntimeError, match=msg):
        ta.update_d_output(np.asarray(ta.time))
    st2 = np.asarray(ta.state).copy()
    st2[:, 1] = configs.outer_ss_state(n, perturb=1e-6, seed=3).reshape(36, n)[:, 1]
    ta.state = st2
    ta.step()
    with pytest.raises(RuntimeError, match=msg):
        ta.tc
    ta.step(write_tc=True)
    tc = np.asarray(ta.tc)
    assert np.all(np.isfinite(tc[:, :, [i for i in range(n) if i != 1]]))


# ---- 3. the dense-output arithmetic against mpmath ----
def _hd(t, thi, tlo, h):
    """The offset of the reference's update_d_output() (src/taylor_adaptive_batch.cpp:2281-2286) and the grid's post-step
    kernel: t - ((t_hi, t_lo) - h) in double-length arithmetic, rounded to double."""
    return ho._df_sub((float(t), 0.0), ho._df_sub((float(thi), float(tlo)), (float(h), 0.0)))[0]


def _eval_restated(c, hd, ha):
    """The dense-output evaluation restated in numpy (plain IEEE operations, no contraction)."""
    c, hd = np.asarray(c, dtype=np.float64), np.float64(hd)
    p = c.shape[-1] - 1
    if ha:
        res, comp, cur = c[..., 0].copy(), np.zeros(c.shape[:-1]), hd
        for k in range(1, p + 1):
            tmp = c[..., k] * cur
            y = tmp - comp
            t = res + y
            comp = (t - res) - y
            res = t
            cur = cur * hd
        return res
    res = c[..., p].copy()
    for k in range(1, p + 1):
        res = c[..., p - k] + res * hd
    return res


def _check_bound(vals, c, hd, hd_exact, ha, label):
    """vals[v] against the exact value of sum_k c[v, k] hd_exact^k (mpmath), within the a-priori bound of the algorithm at
    the double offset hd - Horner: gamma_2p sum |c_k| |hd|^k; compensated sum: (p + 2) eps sum |c_k hd^k| + eps |exact| -
    plus the first-order effect of the rounding of the offset itself, sum k |c_k| |hd|^(k-1) |hd - hd_exact|. Returns the
    largest error as a fraction of the bound."""
    import mpmath as mp

    mp.mp.prec = 240
    p = c.shape[-1] - 1
    u = mp.mpf(EPS) / 2
    gamma = 2 * p * u / (1 - 2 * p * u)
    hde, hdd = mp.mpf(hd_exact), mp.mpf(float(hd))
    dh = abs(hdd - hde)
    ahd = max(abs(hdd), abs(hde))
    worst = 0.0
    for v in range(c.shape[0]):
        cs = [mp.mpf(float(x)) for x in c[v]]
        exact = mp.fsum(cs[k] * hde ** k for k in range(p + 1))
        a_sum = mp.fsum(abs(cs[k]) * ahd ** k for k in range(p + 1))
        d_sum = mp.fsum(k * abs(cs[k]) * ahd ** (k - 1) for k in range(1, p + 1))
        alg = ((p + 2) * mp.mpf(EPS) * a_sum + mp.mpf(EPS) * abs(exact)) if ha else gamma * a_sum
        bound = alg + d_sum * dh * (1 + mp.mpf(2) ** -40) + mp.mpf(2) ** -1074
        err = abs(mp.mpf(float(vals[v])) - exact)
        assert err <= bound, (label, v, float(err), float(bound))
        worst = max(worst, float(err / bound))
    return worst


@pytest.mark.parametrize("which", ["v5", "unrolled"])
def test_update_d_output_against_mpmath_at_offsets_in_and_around_the_step(which):
    """update_d_output(t) after step(write_tc=True), forward and backward, from t ~ 1e4 with a nonzero low part: at hd in
    {0, h/3, h/2, h} and just outside [0, h], within the a-priori bound around the exact value of the integrator's own
    Taylor polynomial at the exact offset (mpmath, from the double-length times)."""
    n = 5
    if which == "v5":
        sys_g, _, st = outer_ss(n, 50)
        ha, mode = True, "v5"
    else:
        st = configs.two_body_state(n, perturb=1e-3, seed=50)
        sys_g, ha, mode = hy.model.nbody(2, masses=[1.0, 0.0]), False, "unrolled"
    import mpmath as mp

    mp.mp.prec = 240
    worst = 0.0
    for backward in (False, True):
        ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=ha, time=1e4)
        _mode(ta, mode)
        for _ in range(3):
            ta.step()
        if backward:
            ta.step_backward(write_tc=True)
        else:
            ta.step(write_tc=True)
        thi, tlo = ta.dtime
        h = np.asarray(ta.last_h)
        assert np.all(tlo != 0.0) and np.all((h < 0) == backward)
        tc = np.asarray(ta.tc)
        for f in (0.0, 1.0 / 3.0, 0.5, 1.0, -1e-3, 1.0 + 1e-3):
            t = np.array([float(mp.mpf(thi[i]) + mp.mpf(tlo[i]) - mp.mpf(h[i]) + mp.mpf(f) * mp.mpf(h[i])) for i in range(n)])
            vals = ta.update_d_output(t)
            for i in range(n):
                hd = _hd(t[i], thi[i], tlo[i], h[i])
                hde = mp.mpf(t[i]) - (mp.mpf(thi[i]) + mp.mpf(tlo[i]) - mp.mpf(h[i]))
                worst = max(worst, _check_bound(vals[:, i], tc[:, :, i], hd, hde, ha, (which, backward, f, i)))
    print("[update_d_output vs mpmath] %s: largest error %.3g of the a-priori bound" % (which, worst))


def test_every_grid_sample_is_the_dense_output_of_the_step_which_spans_its_grid_time():
    """Through a grid callback (one call per sweep, the coefficients of every step), each sweep's coefficients, time and step
    size: every sample must be the dense output of THE step whose range holds its grid time, evaluated at the reference's
    offset - against mpmath within the a-priori bound, and against the same operations restated in numpy. The post-step
    kernel is compiled with -ffp-contract=fast (hiprtc options of csrc/hip_backend.cpp), so bit-identity with the
    restatement is not guaranteed by the language; the test asserts the bound AND the bit-identity it measures. (The callback run is bit-identical to the multi-step run:
    test_gpu_parity.test_propagate_grid_device_loop_with_and_without_callback.)"""
    import mpmath as mp

    n = 5
    sys_g, _, st = outer_ss(n, 51)
    ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=True, time=1e4)
    _mode(ta, "v5")
    for _ in range(2):
        ta.step()
    thi0, _ = ta.dtime
    grid = thi0[None, :] + lane_grid(n, 3.0, 13)
    sweeps = []

    def cb(t):
        hi, lo = t.dtime
        sweeps.append((np.asarray(t.tc).copy(), hi.copy(), lo.copy(), np.asarray(t.last_h).copy()))
        return True

    _, out = ta.propagate_grid(grid, callback=cb)
    assert all(r[0] == OC.time_limit for r in ta.propagate_res) and not np.isnan(out).any()
    n_bit, n_tot, worst = 0, 0, 0.0
    for i in range(n):
        owner = {}
        g = 1
        for s, (_, hi, lo, h) in enumerate(sweeps):
            cur = (hi[i], lo[i])
            st_ = ho._df_sub(cur, (h[i], 0.0))
            t0, t1 = min(cur, st_), max(cur, st_)
            while g < grid.shape[0] and t0 <= (grid[g, i], 0.0) <= t1:
                owner[g] = s
                g += 1
        # (The grid points left over - at most the last one, numerically just outside the last step - belong to the last step
        # of the lane, which reached the end of the grid.)
        last = max(s for s, sw in enumerate(sweeps) if sw[3][i] != 0.0)
        assert g >= grid.shape[0] - 1
        for gg in range(g, grid.shape[0]):
            owner[gg] = last
        for gg, s in owner.items():
            tc, hi, lo, h = sweeps[s]
            hd = _hd(grid[gg, i], hi[i], lo[i], h[i])
            hde = mp.mpf(grid[gg, i]) - (mp.mpf(hi[i]) + mp.mpf(lo[i]) - mp.mpf(h[i]))
            worst = max(worst, _check_bound(out[gg, :, i], tc[:, :, i], hd, hde, True, (i, gg, s)))
            n_bit += int(np.array_equal(_eval_restated(tc[:, :, i], hd, True), out[gg, :, i]))
            n_tot += 1
    print("[grid samples vs mpmath] largest error %.3g of the a-priori bound; %d of %d samples bit-identical to the numpy "
          "restatement" % (worst, n_bit, n_tot))
    # (Measured: every sample. The post-step kernel is built with -ffp-contract=fast, which allows the compiler to fuse the
    # product and the subtraction of the compensated sum; it has not - asserted, so that a toolchain which does shows up.)
    assert n_bit == n_tot


@pytest.mark.parametrize("ha", [False, True])
def test_continuous_output_against_mpmath(ha):
    """continuous_output_batch: the coefficients of the step chosen by the upper bound over the (hi, lo) step times
    (src/continuous_output.cpp:700-842) at the double-length offset tm - times[idx] - inside steps at 0, 1/3, 1/2 and 1 of
    their length and just outside the whole range - within the a-priori bound around mpmath's value of that polynomial at
    the exact offset."""
    import mpmath as mp

    from heyoka_amd import _lib

    n = 5
    rng = np.random.RandomState(53)
    st = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)])
    ta = hy.taylor_adaptive_batch(pendulum(hy), st, n, high_accuracy=ha)
    _mode(ta, "unrolled")
    co, _ = ta.propagate_until(3.0 + 0.1 * np.arange(n), c_output=True)
    ns = co.n_steps
    thi, tlo = np.empty((ns + 2, n)), np.empty((ns + 2, n))
    _lib.raise_for(_lib.lib.hy_cout_get_times(co._h, thi.ctypes.data, tlo.ctypes.data))
    tcs = co.tcs
    mp.mp.prec = 240
    worst = 0.0
    for j in (0, 1, ns // 2, ns - 1):
        for f in (0.0, 1.0 / 3.0, 0.5, 1.0, -1e-3, 1.0 + 1e-3):
            if (f < 0 and j != 0) or (f > 1 and j != ns - 1):
                continue
            tm = np.array([float(mp.mpf(thi[j, i]) + mp.mpf(tlo[j, i]) + mp.mpf(f) * (mp.mpf(thi[j + 1, i]) + mp.mpf(tlo[j + 1, i])
                                                                                     - mp.mpf(thi[j, i]) - mp.mpf(tlo[j, i])))
                           for i in range(n)])
            out = np.asarray(co(tm))
            for i in range(n):
                col = [(thi[k, i], tlo[k, i]) for k in range(ns + 2)]
                first = next(k for k in range(ns + 2) if (tm[i], 0.0) < col[k])
                idx = first - (first != 0) - (first == ns + 1)
                hd = ho._df_sub((tm[i], 0.0), col[idx])[0]
                hde = mp.mpf(tm[i]) - (mp.mpf(col[idx][0]) + mp.mpf(col[idx][1]))
                worst = max(worst, _check_bound(out[:, i], tcs[idx, :, :, i], hd, hde, ha, ("c_output", j, f, i)))
    print("[continuous output vs mpmath] high_accuracy=%s: largest error %.3g of the a-priori bound" % (ha, worst))


# ---- 4.3 the end of a step ----
@pytest.mark.parametrize("build", ["default", "no_contract", "strict"])
@pytest.mark.parametrize("path", ["unrolled", "v5", "staged", "block"])
def test_update_d_output_at_the_end_of_a_step_is_the_state(path, build, monkeypatch):
    """update_d_output(t_end) after step(write_tc=True) - forward and backward, from t = 0 (the offset is then h itself) -
    against the state the step wrote: error in eps of the row's largest entry (rows which are zero: exactly), for the
    position rows and the velocity rows of the N-body state apart. Three builds: the default one, -ffp-contract=off, and
    -ffp-contract=off + kw::exact_division. The reference has the same algorithm in both (src/taylor_00.cpp:808-812,
    src/taylor_01.cpp:1015-1090): bit for bit. Here every stepper is bit for bit without contraction - except the
    straight-line stepper's velocities when they are re-derived from the positions (derive_v: x' = v with v read by no
    node, the two-body test particle; off under kw::exact_division), which the step updates with the derivative of the
    positions' Horner pass plus v^[p] h^p while the dense output evaluates the stored coefficients (k + 1) x^[k+1] with
    Horner: a deviation of rounding size, recorded in DESIGN.md section 2 and asserted here at its measured value. The same
    with a time relative to the current one (rel_time: last_h + t, src/taylor_adaptive_batch.cpp:2276-2280): 0 is the end of
    the step, -h its start - the order-0 coefficients."""
    n = 5
    ha = True
    kw = {"emitter": "table"} if path == "staged" else {}
    if build != "default":
        monkeypatch.setenv("HEYOKA_AMD_HIPRTC_FLAGS", "-ffp-contract=off")
    if build == "strict":
        kw["exact_division"] = True
    if path == "unrolled":
        st = configs.two_body_state(n, perturb=1e-3, seed=52)
        sys_g, ha, mode = hy.model.nbody(2, masses=[1.0, 0.0]), False, "unrolled"
    elif path == "block":
        nb = 12
        masses = list(1.0 / (1.0 + np.arange(nb)) ** 2 * nb / 4.0)
        st = configs.plummer_nbody_state(nb, n, seed=52, jitter=1e-6)
        sys_g, ha, mode = hy.model.nbody(nb, masses=masses), False, "block"
    else:
        sys_g, _, st = outer_ss(n, 52)
        # (kw::exact_division takes the outer Solar System to the lane-pair kernel v3.)
        mode = {"v5": "v3" if build == "strict" else "v5", "staged": "staged"}[path]
    worst = np.zeros(2)  # position rows, velocity rows
    for backward in (False, True):
        ta = hy.taylor_adaptive_batch(sys_g, st, n, high_accuracy=ha, **kw)
        _mode(ta, mode)
        if path == "unrolled":
            # (The re-derived velocities: the derivative pass in the state update - not under kw::exact_division.)
            assert ("der = res + der * h" in ta.hip_source) == (build != "strict")
        if backward:
            ta.step_backward(write_tc=True)
        else:
            ta.step(write_tc=True)
        thi, tlo = ta.dtime
        assert np.all(tlo == 0.0) and np.array_equal(thi, np.asarray(ta.last_h))
        state = np.asarray(ta.state).copy()
        d = ta.update_d_output(thi)
        scale = np.max(np.abs(state), axis=1, keepdims=True)
        assert np.all((scale > 0) | (d == state))
        rows = (np.max(np.abs(d - state) / (np.where(scale > 0, scale, 1.0) * EPS), axis=1)).reshape(-1, 6)
        worst = np.maximum(worst, [np.max(rows[:, :3]), np.max(rows[:, 3:])])
        assert np.array_equal(ta.update_d_output(np.zeros(n), rel_time=True), d)
        assert np.array_equal(ta.update_d_output(-thi, rel_time=True), np.asarray(ta.tc)[:, 0, :])
    print("[update_d_output(t_end) vs state] %s, %s build: positions %.3g eps, velocities %.3g eps of the row scale"
          % (path, build, worst[0], worst[1]))
    # (Measured, positions / velocities. Default build: unrolled 0 / 0.725, v5 1.03 / 0.833, staged 1.03 / 1.09, block 0 / 0 -
    # FMA contraction in the state update or in hy_dout. Without contraction: 0 / 0 everywhere except the re-derived
    # velocities of the unrolled stepper, 0 / 0.725. With kw::exact_division as well: 0 / 0 everywhere.)
    bound = {"default": {"unrolled": (0.0, 0.73), "v5": (1.04, 0.84), "staged": (1.04, 1.1), "block": (0.0, 0.0)},
             "no_contract": {"unrolled": (0.0, 0.73), "v5": (0.0, 0.0), "staged": (0.0, 0.0), "block": (0.0, 0.0)},
             "strict": {"unrolled": (0.0, 0.0), "v5": (0.0, 0.0), "staged": (0.0, 0.0), "block": (0.0, 0.0)}}[build][path]
    assert worst[0] <= bound[0] and worst[1] <= bound[1]
