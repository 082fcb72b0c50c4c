"""callback::angle_reducer on the MI355X. The yardstick is the host-callback path which exists without the feature: the
same integrator with a Python callback applying numpy's unfused x - twopi * floor(x / twopi) through ``ta.state``."""
import copy
import os
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import configs
from heyoka_amd import mixed_models as mm

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
TWOPI = float.fromhex("0x1.921fb54442d18p+2")


def np_reduce(x):
    return x - TWOPI * np.floor(x / TWOPI)


class host_reducer:
    """The reduction restated by hand: what a user had to write before, and the reference for every comparison."""

    def __init__(self, idx):
        self.idx = list(idx)

    def __call__(self, ta):
        st = ta.state
        st[self.idx] = np_reduce(st[self.idx])
        ta.state = st
        return True


def pendula():
    x0, x1, v0, v1 = hy.make_vars("x0", "x1", "v0", "v1")
    return [(x0, v0), (x1, v1), (v0, -hy.sin(x0)), (v1, -hy.sin(x1))], [x0, x1]


def pendula_state(n, seed=11):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(0.0, 2 * np.pi, (2, n)), 10.0 + rng.uniform(0.0, 0.2, (2, n))])


def results(ta):
    oc, mn, mx, ns = ta.propagate_res_arrays()
    hi, lo = ta.dtime
    return dict(state=ta.state, t_hi=hi, t_lo=lo, outcome=np.asarray(oc), min_h=np.asarray(mn), max_h=np.asarray(mx),
                n_steps=np.asarray(ns))


def assert_identical(a, b):
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), (k, a[k], b[k])


def run_pair(make, idx, reducer, t_end, path, **kw):
    """(results with the library's reducer, results with the hand-written host callback, integrator of the former)."""
    ta, tb = make(), make()
    ta.propagate_until(t_end, callback=reducer, **kw)
    assert ta.last_callback_path == path, ta.last_callback_path
    tb.propagate_until(t_end, callback=host_reducer(idx), **kw)
    assert tb.last_callback_path == 1
    return results(ta), results(tb), ta


def check_fused_against_host(make, idx, reducer, t_end, generator, periodic=True):
    logs = []
    hy.set_log_callback(lambda lvl, msg: logs.append(msg))
    try:
        hy.set_logger_level_info()
        ra, rb, ta = run_pair(make, idx, reducer, t_end, 3)
    finally:
        hy.set_logger_level_warn()
        hy.set_log_callback(None)
    assert any("angle_reducer fused into the propagate kernel" in m and generator in m for m in logs), logs
    for k in ("state", "t_hi", "t_lo", "outcome", "n_steps", "min_h", "max_h"):
        print(k, "max |diff| fused vs host callback:",
              float(np.max(np.abs(np.asarray(ra[k], dtype=np.float64) - np.asarray(rb[k], dtype=np.float64)))))
    assert_identical(ra, rb)
    assert np.all(ra["outcome"] == int(hy.taylor_outcome.time_limit)) and np.all(ra["n_steps"] > 5)
    fl = ra["state"][idx]
    assert np.all(fl >= 0.0) and np.all(fl <= TWOPI) and np.all(fl <= 2 * np.pi)
    # Unflagged variables against a run without any callback: the project's default-build tolerance (sin sees other
    # arguments, so not bit for bit). Only where a shift of one angle by 2 pi is a symmetry of the equations (`periodic`).
    if not periodic:
        return ta
    tn = make()
    tn.propagate_until(t_end)
    assert tn.last_callback_path == 0
    un = [i for i in range(ta.dim) if i not in idx]
    ref = tn.state[un]
    assert np.max(np.abs(ra["state"][un] - ref) / np.maximum(1.0, np.abs(ref))) <= 1e6 * EPS
    return ta


@pytest.mark.parametrize("n", [1, 3, 64, 65])
@pytest.mark.parametrize("emitter", [None, "unrolled"])
def test_fused_reduction_is_bit_identical_to_the_host_callback(n, emitter):
    """Two uncoupled rotating pendula, angles over [0, 2 pi), {x0, x1} reduced, propagate_until(20): states, times,
    outcomes, step counts and min / max |h| of the fused launch equal those of the host-callback loop bit for bit, at one
    wavefront's worth of systems and its neighbours. With the default generator (two pendula: the first-generation
    wave-cluster kernel, two lanes per system) and with the straight-line one."""
    sys_, ang = pendula()
    st = pendula_state(n)
    kw = {} if emitter is None else {"emitter": emitter}
    make = lambda: hy.taylor_adaptive_batch(sys_, st, n, **kw)  # noqa: E731
    ta = check_fused_against_host(make, [0, 1], hy.callback.angle_reducer(ang), 20.0,
                                  "unrolled" if emitter else "cluster")
    assert ("unrolled" in ta.hip_source_mode) == (emitter == "unrolled")


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_fused_reduction_on_the_table_steppers(n, lds, monkeypatch):
    monkeypatch.setenv("HEYOKA_AMD_TABLE_LDS", lds)
    sys_, ang = pendula()
    st = pendula_state(n, seed=5)
    make = lambda: hy.taylor_adaptive_batch(sys_, st, n, emitter="table")  # noqa: E731
    ta = check_fused_against_host(make, [0, 1], hy.callback.angle_reducer(ang), 20.0, "table")
    assert ("table mode (staged)" in ta.hip_source_mode) == (lds == "1") and ("tape in HBM" in ta.hip_source_mode) == (lds == "0")


@pytest.mark.parametrize("sites,n", [(4, 1), (4, 3), (4, 5), (16, 1), (16, 3), (16, 5)])
def test_fused_reduction_on_the_sine_lattice(sites, n):
    """mixed_models.sine_lattice, angles offset by +40 so that the reduction acts. 4 sites: the planner keeps so small a
    chain on the straight-line generator; 16 sites: the multi-class wave-cluster generator, 4 systems per wavefront - 5
    systems are one full group and a partial one.
    The assertions of the pendulum test, but one: the comparison of the unflagged variables with a run WITHOUT a callback
    is left out here, because it cannot hold for this system - the bonds k d + beta d^3, d = th_(i+1) - th_i, are not periodic
    in the angles, so reducing the angles one by one changes the forces as soon as one of them wraps (measured on an MI355X:
    angular velocities 7.9 ... 19 apart after t = 3, while fused and host-callback runs agree bit for bit)."""
    st = mm.sine_lattice_state(sites, n, seed=3)
    st[:sites] += 40.0
    sys_ = mm.sine_lattice(hy, sites)
    make = lambda: hy.taylor_adaptive_batch(sys_, st, n)  # noqa: E731
    red = hy.callback.angle_reducer([v for v, _ in sys_[:sites]])
    ta = check_fused_against_host(make, list(range(sites)), red, 3.0, "classes of clusters" if sites == 16 else "unrolled",
                                  periodic=False)
    assert ("classes of clusters" in ta.hip_source_mode) == (sites == 16)


def test_generators_without_the_variant_fall_back_to_a_reduction_per_sweep():
    """The outer Solar System on the one-lane-per-pair kernel with a reducer on one coordinate (physically meaningless: it
    exercises the decline): path 2, the host-callback results bit for bit, the stepper's source untouched."""
    n = 3
    oss = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
    st = configs.outer_ss_state(n, perturb=1e-8, seed=11)
    make = lambda: hy.taylor_adaptive_batch(oss, st, n, high_accuracy=True)  # noqa: E731
    src0 = make().hip_source
    logs = []
    hy.set_log_callback(lambda lvl, msg: logs.append(msg))
    try:
        hy.set_logger_level_info()
        ra, rb, ta = run_pair(make, [6], hy.callback.angle_reducer([oss.vars[6]]), 2.0, 2)
    finally:
        hy.set_logger_level_warn()
        hy.set_log_callback(None)
    assert any("hy_angle_reduce after every sweep" in m and "v5" in m for m in logs), logs
    assert "v5" in ta.hip_source_mode and ta.hip_source == src0 and "hy_angle_red" not in src0
    assert_identical(ra, rb)
    assert np.all(ra["n_steps"] >= 2)


@pytest.mark.parametrize("family,path", [("unrolled", 3), ("cluster", 3), ("staged", 3), ("hbm_tape", 3), ("multi_class", 3),
                                         ("v5_declines", 2)])
def test_a_system_which_takes_no_step_is_reduced_once(family, path, monkeypatch):
    """Per-lane final times [t0, t0 + 5, t0 + 5], the angle of lane 0 at 50: after the call it is reduced and its time is
    unchanged - on every generator with a fused variant (path 3) and on the per-sweep path (2)."""
    n, t0 = 3, 1.5
    if family == "v5_declines":
        sys_ = hy.model.nbody(6, masses=configs.OUTER_SS_MASSES, Gconst=configs.OUTER_SS_G)
        st = configs.outer_ss_state(n, perturb=1e-8, seed=11)
        kw, idx, want = {"high_accuracy": True}, [6], "v5"
        red = hy.callback.angle_reducer([sys_.vars[6]])
    elif family == "multi_class":
        sys_ = mm.sine_lattice(hy, 16)
        st = mm.sine_lattice_state(16, n, seed=3)
        kw, idx, want = {}, list(range(16)), "classes of clusters"
        red = hy.callback.angle_reducer([v for v, _ in sys_[:16]])
    else:
        sys_, ang = pendula()
        st = pendula_state(n)
        red, idx = hy.callback.angle_reducer(ang), [0, 1]
        kw = {"unrolled": {"emitter": "unrolled"}, "cluster": {}}.get(family, {"emitter": "table"})
        want = {"unrolled": "unrolled", "cluster": "cluster mode", "staged": "table mode (staged)", "hbm_tape": "tape in HBM"}[family]
        if family in ("staged", "hbm_tape"):
            monkeypatch.setenv("HEYOKA_AMD_TABLE_LDS", "1" if family == "staged" else "0")
    row = idx[0]
    st[row, 0] = 50.0
    make = lambda: hy.taylor_adaptive_batch(sys_, st, n, time=t0, **kw)  # noqa: E731
    tf = np.array([t0, t0 + 5.0, t0 + 5.0])
    ra, rb, ta = run_pair(make, idx, red, tf, path)
    assert want in ta.hip_source_mode, ta.hip_source_mode
    assert_identical(ra, rb)
    assert ra["state"][row, 0] == np_reduce(np.float64(50.0)) and ra["t_hi"][0] == t0 and ra["n_steps"][0] == 0
    assert np.array_equal(ra["t_hi"], tf) and np.all(ra["n_steps"][1:] > 0)


def test_sets_continuous_output_grids_and_events_use_the_reduction_per_sweep():
    sys_, ang = pendula()
    x0 = ang[0]
    n = 3
    st = pendula_state(n, seed=7)
    make = lambda **kw: hy.taylor_adaptive_batch(sys_, st, n, **kw)  # noqa: E731

    # A set with a user callback (the reference's batch test, restated): host callback loop, reduction on the device.
    def in_range(ta):
        s = ta.state[:2]
        assert np.all(s >= 0.0) and np.all(s < 6.29)
        return True

    ta, tb = make(), make()
    ta.propagate_until(20.0, callback=[hy.callback.angle_reducer(ang), in_range])
    tb.propagate_until(20.0, callback=[host_reducer([0, 1]), in_range])
    assert ta.last_callback_path == 1
    assert_identical(results(ta), results(tb))
    # Two reducers in a set are still a pure reducer: fused, the union of their indices.
    tc = make()
    tc.propagate_until(20.0, callback=[hy.callback.angle_reducer(ang[:1]), hy.callback.angle_reducer(ang[1:])])
    assert tc.last_callback_path == 3
    assert_identical(results(tc), results(tb))
    # Continuous output.
    ta, tb = make(), make()
    ca, _ = ta.propagate_until(5.0, callback=hy.callback.angle_reducer(ang), c_output=True)
    cb, _ = tb.propagate_until(5.0, callback=host_reducer([0, 1]), c_output=True)
    assert ta.last_callback_path == 2
    assert_identical(results(ta), results(tb))
    assert np.array_equal(ca(np.full(n, 2.5)), cb(np.full(n, 2.5)))
    # propagate_grid, 5 points.
    grid = np.linspace(0.0, 5.0, 5)
    ta, tb = make(), make()
    _, oa = ta.propagate_grid(grid, callback=hy.callback.angle_reducer(ang))
    _, ob = tb.propagate_grid(grid, callback=host_reducer([0, 1]))
    assert ta.last_callback_path == 2
    assert np.array_equal(oa.view(np.uint64), ob.view(np.uint64))
    assert_identical(results(ta), results(tb))
    # One non-terminal counting event.
    ca_, cb_ = hy.native_event_counter(), hy.native_event_counter()
    ta = make(nt_events=[hy.nt_event(hy.sin(x0), ca_)])
    tb = make(nt_events=[hy.nt_event(hy.sin(x0), cb_)])
    ta.propagate_until(5.0, callback=hy.callback.angle_reducer(ang))
    tb.propagate_until(5.0, callback=host_reducer([0, 1]))
    assert ta.last_callback_path == 2
    assert_identical(results(ta), results(tb))
    assert ca_.value == cb_.value and ca_.value > 0


def test_energy_of_the_pendula_is_conserved_with_the_reduction():
    """The reference's own bound (test/angle_reducer.cpp): 1000 eps after propagate_until(100)."""
    sys_, ang = pendula()
    st = np.array([[0.05, 0.06], [0.05, 0.05], [10.0, 10.01], [10.1, 10.11]])
    energy = lambda s: 0.5 * s[2:] ** 2 + (1.0 - np.cos(s[:2]))  # noqa: E731
    ta = hy.taylor_adaptive_batch(sys_, st, 2)
    ta.propagate_until(100.0, callback=hy.callback.angle_reducer(ang))
    assert ta.last_callback_path == 3
    e0, e1 = energy(st), energy(ta.state)
    assert np.all(np.abs(e1 - e0) <= 1000.0 * EPS * np.abs(e0)), (e1 - e0) / (EPS * e0)
    assert np.all(ta.state[:2] >= 0.0) and np.all(ta.state[:2] < 6.29)


def test_errors_on_the_device_path():
    sys_, ang = pendula()
    ta = hy.taylor_adaptive_batch(sys_, pendula_state(2), 2)
    msg = "Cannot use an angle_reducer which was default-constructed or moved-from"
    with pytest.raises(ValueError) as e:
        ta.propagate_until(1.0, callback=hy.callback.angle_reducer())
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        hy.callback.angle_reducer()(ta)
    assert str(e.value) == msg
    _, cb = ta.propagate_until(1.0, callback=hy.callback.angle_reducer(ang[1:]))
    x0 = hy.make_vars("x0")
    t1 = hy.taylor_adaptive_batch([(x0, x0)], np.array([[0.05, 0.06]]), 2)
    with pytest.raises(ValueError) as e:
        cb(t1)
    assert str(e.value) == ("Inconsistent state detected in angle_reducer: the last index in the indices vector has a value "
                            "of 1, but the number of state variables is only 1")


def test_step_after_a_fused_propagation_does_not_reduce_and_a_lone_call_does():
    sys_, ang = pendula()
    ta = hy.taylor_adaptive_batch(sys_, pendula_state(3), 3, emitter="unrolled")
    red = hy.callback.angle_reducer(ang)
    ta.propagate_until(2.0, callback=red)
    assert ta.last_callback_path == 3
    st = ta.state
    st[0] = 50.0
    ta.state = st
    ta.step()
    assert np.all(np.abs(ta.state[0] - 50.0) < 2.0)
    # Stand-alone: host copy newer (just set), then device copy newer (after a step) - getters see reduced values.
    st = ta.state
    st[1] = -3.0
    ta.state = st
    assert red(ta) is True
    assert np.array_equal(ta.state[1], np_reduce(np.full(3, -3.0)))
    ta.step()
    before = ta.state
    red(ta)
    assert np.array_equal(ta.state[:2], np_reduce(before[:2])) and np.array_equal(ta.state[2:], before[2:])


def test_cpp_interface_on_gpu():
    from test_angle_reducer import build_cpp

    out = subprocess.run([build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "angle_reducer GPU checks OK" in out.stdout
