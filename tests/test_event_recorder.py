"""The event log: library-side recording callbacks (hy_event_recorder_nt / hy_event_recorder_t, native_event_recorder)
whose rows - system, class, event index, d_sgn, trigger time (hi, lo), root, |d eq/dt|, state at the trigger time - are
written on the device, in the order in which the host loop would have invoked the callbacks.

What the GPU tests hold the log to:
- the device path against the host loop (Python callbacks appending the same data), bit for bit and in order;
- the mixed path (a recorder next to a host callback: the host loop collects the headers) against the device path, whole
  rows, bit for bit;
- the state columns: terminal rows against the state after the step, bit for bit; non-terminal rows against the exact
  value (mpmath) of the integrator's own Taylor polynomial at the root, within the a-priori bound of the evaluation
  algorithm - the bounds tests/test_grid_parity.py derives, restated in _state_bound();
- the oracle's callback sequence;
- the edges of the two-level scan (second-level passes of 65 536 lanes, empty workgroups, a partial last workgroup,
  several rows per lane, growth of the log);
- the life cycle of the log."""
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import _lib, configs
from conftest import EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OC = hy.taylor_outcome


def _pendulum():
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -9.8 * hy.sin(x))], x, v


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_ta(**kw):
    sys_, x, v = _pendulum()
    rec = [hy.native_event_recorder() for _ in range(3)]
    ta = hy.taylor_adaptive_batch(sys_, [[0.1] * 4, [0.2] * 4], 4,
                                  nt_events=[hy.nt_event(v, rec[0]), hy.nt_event(x - 0.3, rec[1])],
                                  t_events=[hy.t_event(x + 0.3, rec[2], cooldown=0.05)], **kw)
    return ta, rec


def test_recorder_integrator_constructs_without_a_gpu_and_has_an_empty_log():
    ta, rec = _cpu_ta()
    assert ta.with_events and ta.event_log_size == 0 and ta.event_log_capacity == 0
    assert ta.event_log_row_size == 8 + ta.dim == 10
    assert ta.event_log_states
    log = ta.event_log
    assert len(log) == 0 and log.state.shape == (0, 2) and log.system.shape == (0,)
    assert [r.value for r in rec] == [0, 0, 0]
    ta.event_log_states = False
    assert ta.event_log_row_size == 8 and ta.event_log.state is None
    ta.event_log_states = True
    assert ta.event_log_row_size == 10
    # The copy: same switch, empty log.
    ta.event_log_states = False
    c = ta.copy()
    assert c.event_log_size == 0 and c.event_log_row_size == 8
    # Without a device nothing is allocated: reserve / clear / the zero-copy view of an empty log.
    ta.event_log_reserve(1000)
    ta.clear_event_log()
    assert ta.event_log_size == 0 and ta.event_log_device is None
    with pytest.raises(Exception, match="range"):
        ta.get_event_log(0, 1)


def test_integrator_without_recorders_has_no_log_and_no_recorder_kernels():
    sys_, x, v = _pendulum()
    ta = hy.taylor_adaptive_batch(sys_, None, 4, nt_events=[hy.nt_event(v, hy.native_event_counter())])
    assert ta.event_log_size == 0 and ta.event_log_capacity == 0 and ta.event_log_device is None
    with pytest.raises(Exception, match="no recording event callbacks"):
        ta.event_log_code_object(0)


def test_states_switch_is_validated():
    """The switch is refused on a non-empty log (hy_tab_set_event_log_states: error code + message; the GPU life-cycle test
    drives that path); without a device the log is always empty, so here: the round trip, and the C call's return codes."""
    ta, _ = _cpu_ta()
    lib = _lib.lib
    assert lib.hy_tab_set_event_log_states(ta._h, 0) == 0 and lib.hy_tab_get_event_log_states(ta._h) == 0
    assert lib.hy_tab_set_event_log_states(ta._h, 0) == 0
    assert lib.hy_tab_set_event_log_states(ta._h, 1) == 0 and lib.hy_tab_get_event_log_states(ta._h) == 1


def test_recorder_modules_compile_for_gfx950_and_name_the_new_kernels():
    _lib.raise_for(_lib.lib.hy_compile_aux_kernels(20, 2, 0))
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    y1, y3 = hy.make_vars("y_1", "y_3")
    oss = hy.model.nbody(6, masses=M, Gconst=G)
    tas = [_cpu_ta()[0], _cpu_ta(high_accuracy=True)[0]]
    for kw in ({}, {"cluster_kernel": "v2"}):
        for ha in (False, True):
            tas.append(hy.taylor_adaptive_batch(oss, None, 64, high_accuracy=ha, nt_events=[hy.nt_event(y1, hy.native_event_recorder())],
                                                t_events=[hy.t_event(y3, hy.native_event_recorder(), cooldown=0.05)], **kw))
    assert "inside the stepper" in tas[2].hip_source_mode and "v2" in tas[4].hip_source_mode
    for ta in tas:
        hdr, dout = ta.event_log_code_object(0), ta.event_log_code_object(1)
        assert hdr[:4] == b"\x7fELF" and dout[:4] == b"\x7fELF"
        for k in (b"hy_evr_count", b"hy_evr_scan", b"hy_evr_write"):
            assert k in hdr and k not in dout
        assert b"hy_dout_rows" in dout and b"hy_dout_rows" not in hdr
        assert b"gfx950" in hdr and b"gfx950" in dout
        # (The stepper's module is the one of the same integrator with host callbacks: nothing of the log in it.)
        assert b"hy_evr_" not in ta.code_object and b"hy_dout_rows" not in ta.code_object


def test_event_detection_source_without_recorders_is_unchanged():
    """The HIP source of the event-detection module against the hashes recorded from the commit before the event log
    (tests/golden/event_detection_source_sha256.json)."""
    with open(os.path.join(ROOT, "tests", "golden", "event_detection_source_sha256.json")) as f:
        gold = json.load(f)
    keys = [k for k in gold if k != "comment"]
    assert len(keys) >= 4
    for k in keys:
        order, n_te, n_nte = (int(s) for s in k.split())
        src = _lib.take_str(_lib.lib.hy_event_detection_source(order, n_te, n_nte))
        assert "hy_evr_" not in src and "hy_dout_rows" not in src
        assert hashlib.sha256(src.encode()).hexdigest() == gold[k], k


EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_event_recorder")


def _build_cpp():
    """tests/cpp/test_event_recorder.cpp, compiled the way tests/test_cpp_api.py compiles its programs."""
    src = os.path.join(ROOT, "tests", "cpp", "test_event_recorder.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_event_recorder_host_half():
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_cpp_event_recorder_on_gpu():
    out = subprocess.run([_build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
CONFIGS = ["pendulum", "outer_ss_v5", "outer_ss_v2"]
N_SYS, N_STEPS = 1024, 12
# Steps after which the Taylor coefficients are fetched from integrator A (test 3): late ones, so that most of the run
# happens before anybody has asked for them.
TC_STEPS = (8, 11)
MAX_TC_LANES = 12


@functools.lru_cache(maxsize=None)
def _outer_ss_spread():
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    rng = np.random.RandomState(5)
    sysd = hy.model.nbody(6, masses=M, Gconst=G)
    spread = hy.taylor_adaptive_batch(sysd, configs.outer_ss_state(N_SYS, perturb=1e-6, seed=31), N_SYS, high_accuracy=True)
    spread.propagate_until(rng.uniform(0.0, 30.0, N_SYS))
    return sysd, np.array(spread.state)


def _setup(config):
    """(system, state, non-terminal event equations, terminal event equation, keyword arguments): the ensemble of
    test_library_side_counting_callbacks_are_applied_on_the_device for the outer Solar System, an analogous one - random
    phases and amplitudes, two plane crossings and a terminal one with cooldown 0.05 - for the pendulum."""
    if config == "pendulum":
        sys_, x, v = _pendulum()
        rng = np.random.RandomState(11)
        st = np.stack([rng.uniform(-1.4, 1.4, N_SYS), rng.uniform(-2.0, 2.0, N_SYS)])
        return sys_, st, [v, x - 0.02], x + 0.03, {}
    sysd, st = _outer_ss_spread()
    y1, y2, y3 = hy.make_vars("y_1", "y_2", "y_3")
    return sysd, st, [y1, y2], y3, ({} if config == "outer_ss_v5" else {"cluster_kernel": "v2"})


class _HostLog:
    """Python callbacks which append what a recorder records of an event: (lane, class, idx, d_sgn, time). A terminal
    callback receives no time: NaN here, checked against the lane's time after the step."""

    def __init__(self):
        self.rows = []

    def nt(self, k):
        return lambda ta, t, d_sgn, idx: self.rows.append((idx, 1, k, d_sgn, t))

    def t(self, k):
        return lambda ta, d_sgn, idx: self.rows.append((idx, 0, k, d_sgn, np.nan)) or True


@functools.lru_cache(maxsize=None)
def _run(config, ha):
    """A: recorders on every event (device path). B: Python callbacks (host loop). C: A with a do-nothing Python callback in
    place of the recorder of the second non-terminal event (host loop which collects the recorders' headers). Twelve steps
    in lock step; everything the tests compare is kept per step."""
    sys_, st, nt_eqs, t_eq, kw = _setup(config)
    n = st.shape[1]
    rec = [hy.native_event_recorder() for _ in range(3)]
    a = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=ha, nt_events=[hy.nt_event(nt_eqs[0], rec[0]), hy.nt_event(nt_eqs[1], rec[1])],
                                 t_events=[hy.t_event(t_eq, rec[2], cooldown=0.05)], **kw)
    hl = _HostLog()
    b = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=ha, nt_events=[hy.nt_event(nt_eqs[0], hl.nt(0)), hy.nt_event(nt_eqs[1], hl.nt(1))],
                                 t_events=[hy.t_event(t_eq, hl.t(0), cooldown=0.05)], **kw)
    c = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=ha,
                                 nt_events=[hy.nt_event(nt_eqs[0], hy.native_event_recorder()), hy.nt_event(nt_eqs[1], lambda *args: None)],
                                 t_events=[hy.t_event(t_eq, hy.native_event_recorder(), cooldown=0.05)], **kw)
    # (C2: the Python callback on the FIRST non-terminal event instead, so that the rows of every event of the device
    # path - time_lo, root and |d eq/dt| included - meet rows built by the host loop from the records of the step.)
    c2 = hy.taylor_adaptive_batch(sys_, st, n, high_accuracy=ha,
                                  nt_events=[hy.nt_event(nt_eqs[0], lambda *args: None), hy.nt_event(nt_eqs[1], hy.native_event_recorder())],
                                  t_events=[hy.t_event(t_eq, hy.native_event_recorder(), cooldown=0.05)], **kw)
    mode = a.hip_source_mode
    steps = []
    for s in range(N_STEPS):
        n0, nb0 = a.event_log_size, len(hl.rows)
        a.step()
        b.step()
        c.step()
        c2.step()
        new = a.get_event_log(n0)
        d = {"a_rows": new.rows, "b_rows": np.array(hl.rows[nb0:], dtype=float).reshape(-1, 5),
             "step_res": (a.step_res, b.step_res, c.step_res),
             "state": (np.array(a.state), np.array(b.state), np.array(c.state)),
             "time": (np.array(a.time), np.array(b.time), np.array(c.time)),
             "cd": (a.te_cooldowns, b.te_cooldowns, c.te_cooldowns)}
        if s in TC_STEPS:
            lanes = np.unique(new.system[~new.terminal])[:MAX_TC_LANES]
            d["tc_lanes"] = lanes
            d["tc"] = np.array(a.tc)[:, :, lanes]
            # The integrator's own dense output (update_d_output(): hy_dout on the full coefficients) at the root of the
            # first non-terminal row of every lane which has one. Relative times are offsets from the END of the step,
            # h' = last_h + t: only the lanes in which last_h + (root - last_h) gives the root back exactly take part.
            nt_rows = new.rows[~new.terminal]
            lanes_u, first = np.unique(nt_rows[:, 0].astype(int), return_index=True)
            h = np.array([hh for _, hh in d["step_res"][0]])
            t_rel = np.zeros(n)
            t_rel[lanes_u] = nt_rows[first, 6] - h[lanes_u]
            ok = h[lanes_u] + t_rel[lanes_u] == nt_rows[first, 6]
            d["dout_ref"] = a.update_d_output(t_rel, rel_time=True)[:, lanes_u[ok]].T
            d["dout_rows"] = nt_rows[first][ok][:, 8:]
        steps.append(d)
    return {"mode": mode, "steps": steps, "a_log": a.event_log.rows, "c_log": c.event_log.rows, "c2_log": c2.event_log.rows, "dim": a.dim, "order": a.order,
            "counts": [r.value for r in rec]}


def _check_mode(config, mode):
    if config == "pendulum":
        assert "unrolled" in mode, mode
    elif config == "outer_ss_v5":
        assert "v5" in mode and "inside the stepper" in mode, mode
    else:
        assert "v2" in mode and "inside the stepper" not in mode, mode


@pytest.mark.gpu
@pytest.mark.parametrize("ha", [True, False])
@pytest.mark.parametrize("config", CONFIGS)
def test_device_path_equals_host_loop_bit_for_bit(config, ha):
    """Test 1. After every step: step_res, states, times and cooldowns of A and B are equal, and columns 0-4 of A's new
    rows (system, class, idx, d_sgn, time hi) equal B's list in order. The trigger time of a terminal event is not handed to
    a host callback: that column of a terminal row is checked against the lane's time after the step - the step ends at the
    event, and the double-length (t - h) + h reproduces t unless t lies within 2^-104 relative of a rounding boundary."""
    r = _run(config, ha)
    _check_mode(config, r["mode"])
    n_rows = n_term = 0
    for s, d in enumerate(r["steps"]):
        assert d["step_res"][0] == d["step_res"][1], s
        assert np.array_equal(d["state"][0], d["state"][1]) and np.array_equal(d["time"][0], d["time"][1]), s
        assert d["cd"][0] == d["cd"][1], s
        ar, br = d["a_rows"], d["b_rows"]
        assert ar.shape[0] == br.shape[0], (s, ar.shape, br.shape)
        assert np.array_equal(ar[:, :4], br[:, :4]), s
        term = ar[:, 1] == 0.0
        assert np.array_equal(ar[~term, 4], br[~term, 4]), s
        assert np.all(np.isnan(br[term, 4]))
        assert np.array_equal(ar[term, 4], d["time"][0][ar[term, 0].astype(int)]), s
        # (Batch order, and at most one terminal row per lane and step - the last of the lane's rows.)
        assert np.all(np.diff(ar[:, 0]) >= 0)
        n_rows += ar.shape[0]
        n_term += int(np.sum(term))
    assert n_rows > 100 and n_term > 10, (n_rows, n_term)
    print("[event log, device path vs host loop] %s ha=%s: %d rows, %d terminal" % (config, ha, n_rows, n_term))
    # Counters handed over through `user`: invocations per event.
    al = r["a_log"]
    assert r["counts"] == [int(np.sum((al[:, 1] == 1) & (al[:, 2] == 0))), int(np.sum((al[:, 1] == 1) & (al[:, 2] == 1))),
                           int(np.sum(al[:, 1] == 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("ha", [True, False])
@pytest.mark.parametrize("config", CONFIGS)
def test_mixed_path_equals_device_path(config, ha):
    """Test 2. C (host loop, headers collected where the recorders' callbacks run) against A (device path) with the rows of
    the event which has a Python callback in C removed: whole rows - headers, root, |d eq/dt|, states - bit for bit. C has
    the Python callback on the second non-terminal event, C2 on the first: between them every row of A is compared."""
    r = _run(config, ha)
    for s, d in enumerate(r["steps"]):
        assert d["step_res"][0] == d["step_res"][2] and np.array_equal(d["state"][0], d["state"][2]), s
        assert np.array_equal(d["time"][0], d["time"][2]) and d["cd"][0] == d["cd"][2], s
    al, cl = r["a_log"], r["c_log"]
    keep = ~((al[:, 1] == 1) & (al[:, 2] == 1))
    assert 0 < np.sum(keep) < al.shape[0] and cl.shape[1] == 8 + r["dim"]
    assert cl.shape[0] == np.sum(keep)
    assert np.array_equal(al[keep], cl)
    keep2 = ~((al[:, 1] == 1) & (al[:, 2] == 0))
    assert 0 < np.sum(keep2) < al.shape[0] and np.array_equal(al[keep2], r["c2_log"])


def _state_bound(c, root, ha):
    """A-priori bound of the dense-output evaluation of sum_k c[k] root^k in double precision, and the exact value (mpmath).
    Horner (high_accuracy off): gamma_2p sum |c_k| |root|^k with gamma_n = n u / (1 - n u), u = eps / 2 (Higham, Accuracy
    and Stability of Numerical Algorithms, section 5.1). Compensated sum of the terms c_k root^k with the running power
    (high_accuracy on): every term carries at most k roundings - (p + 1) eps sum |c_k root^k| with the summation's own
    first-order eps |exact| and its second-order term folded into (p + 2). The bounds of tests/test_grid_parity.py; the
    offset is the double in the row, so its rounding does not enter."""
    import mpmath as mp

    mp.mp.prec = 240
    p = len(c) - 1
    u = mp.mpf(EPS) / 2
    gamma = 2 * p * u / (1 - 2 * p * u)
    h = mp.mpf(float(root))
    cs = [mp.mpf(float(x)) for x in c]
    exact = mp.fsum(cs[k] * h ** k for k in range(p + 1))
    a_sum = mp.fsum(abs(cs[k]) * abs(h) ** k for k in range(p + 1))
    bound = ((p + 2) * mp.mpf(EPS) * a_sum + mp.mpf(EPS) * abs(exact)) if ha else gamma * a_sum
    return exact, bound + mp.mpf(2) ** -1074


@pytest.mark.gpu
@pytest.mark.parametrize("ha", [True, False])
@pytest.mark.parametrize("config", CONFIGS)
def test_state_columns(config, ha):
    """Test 3. Terminal rows: the lane's column of the state right after the step, bit for bit (every step). Non-terminal
    rows (the steps whose Taylor coefficients were fetched, a dozen lanes each): the integrator's own polynomial at the root,
    within the a-priori bound of the evaluation algorithm. root and |d eq/dt| against the host loop: test 2 compares
    them with C's rows, which the host loop built from the records of the step."""
    import mpmath as mp

    r = _run(config, ha)
    n_term = n_nt = 0
    worst = 0.0
    for s, d in enumerate(r["steps"]):
        ar = d["a_rows"]
        term = ar[:, 1] == 0.0
        lanes = ar[term, 0].astype(int)
        assert np.array_equal(ar[term, 8:], d["state"][0][:, lanes].T), s
        n_term += lanes.size
        if "tc" not in d:
            continue
        pos = {int(l): i for i, l in enumerate(d["tc_lanes"])}
        for row in ar[~term]:
            if int(row[0]) not in pos:
                continue
            tc = d["tc"][:, :, pos[int(row[0])]]
            for v in range(r["dim"]):
                exact, bound = _state_bound(tc[v], row[6], ha)
                err = abs(mp.mpf(float(row[8 + v])) - exact)
                assert err <= bound, (config, ha, s, int(row[0]), v, float(err), float(bound))
                worst = max(worst, float(err / bound))
            n_nt += 1
    assert n_term > 10 and n_nt >= 10, (n_term, n_nt)
    print("[event log states vs mpmath] %s ha=%s: %d non-terminal rows, largest error %.3g of the a-priori bound; %d terminal "
          "rows bit-identical to the state" % (config, ha, n_nt, worst, n_term))


@pytest.mark.gpu
@pytest.mark.parametrize("ha", [True, False])
@pytest.mark.parametrize("config", CONFIGS)
def test_state_columns_equal_the_dense_output_of_the_integrator(config, ha):
    """hy_dout_rows restates the evaluation of hy_dout (and, on compact coefficients, of hy_dout_c, which promises the
    operations and operation order of hy_dout on the full set): the state columns of non-terminal rows against
    update_d_output() at the same offset, bit for bit."""
    r = _run(config, ha)
    n_cmp = 0
    for d in r["steps"]:
        if "dout_ref" in d:
            assert np.array_equal(d["dout_rows"], d["dout_ref"])
            n_cmp += d["dout_rows"].shape[0]
    assert n_cmp >= 10, n_cmp
    print("[event log states vs update_d_output] %s ha=%s: %d rows bit-identical" % (config, ha, n_cmp))


@pytest.mark.gpu
def test_log_against_the_oracle():
    """Test 4. The ensemble and the steps of test_events_batch_vs_oracle: the (system, class, idx, d_sgn) sequence of the log
    is the oracle's callback sequence; trigger times within that test's tolerance (1e-12) - the oracle's terminal callback
    receives no time, so those of the non-terminal rows."""
    import heyoka_oracle as ho

    n = 7
    amp = np.linspace(0.05, 1.2, n)
    st = np.stack([-amp, np.zeros(n)])
    sys_, x, v = _pendulum()
    ox, ov = ho.var("x"), ho.var("v")
    seq = []
    ta = hy.taylor_adaptive_batch(
        sys_, st, n,
        nt_events=[hy.nt_event(v, hy.native_event_recorder()),
                   hy.nt_event(x, hy.native_event_recorder(), direction=hy.event_direction.negative)],
        t_events=[hy.t_event(x * x + v * v - 1e-3, hy.native_event_recorder(), cooldown=0.05)])
    ora = ho.OracleEventIntegrator(
        [(ox, ov), (ov, -9.8 * ho.sin(ox))], st, n,
        nt_events=[ho.nt_event(ov, lambda ta, t, d, i: seq.append((i, 1, 0, d, t))),
                   ho.nt_event(ox, lambda ta, t, d, i: seq.append((i, 1, 1, d, t)), direction=ho.DIR_NEGATIVE)],
        t_events=[ho.t_event(ox * ox + ov * ov - 1e-3, lambda ta, d, i: seq.append((i, 0, 0, d, np.nan)) or True, cooldown=0.05)])
    for _ in range(12):
        ta.step()
        ora.step()
        assert [int(oc) for oc, _ in ta.step_res] == [oc for oc, _ in ora.step_res]
    log = ta.event_log
    seq = np.array(seq, dtype=float).reshape(-1, 5)
    assert len(log) == seq.shape[0] > 10
    assert np.array_equal(log.rows[:, :4], seq[:, :4])
    nt = ~log.terminal
    assert np.max(np.abs(log.time[nt] - seq[nt, 4])) <= 1e-12
    assert np.all(np.abs(log.time_lo) <= np.abs(log.time) * EPS)


# Test 5. One pass of the second-level scan (hy_evr_scan: one workgroup, 256 workgroup sums per pass) covers
# 256 * 256 = 65 536 lanes: N just above that takes two passes, with a partial last workgroup of 300 - 256 = 44 lanes.
SCAN_N = 65536 + 300
SCAN_STEPS = 6
SCAN_THR = (0.3, 0.3001, 0.3002)


def _scan_state(n=SCAN_N):
    """Workgroups of 256 consecutive systems, one in four active, and the last two (the full one from 65 536 and the
    partial one behind it): pendulums swinging up through the three close thresholds (three rows of one lane in one step), at
    different times - under half of them within the first step, which sizes the log -, turning (v = 0) and coming back
    down through them; some start above the thresholds. The others rotate (|v| above the separatrix, 2 sqrt(9.8) = 6.3): x grows for ever from 1, v never
    vanishes - no event, no row."""
    rng = np.random.RandomState(3)
    j = np.arange(n)
    active = ((j // 256) % 4 == 0) | (j >= 65536)
    x = np.where(active, rng.uniform(-0.5, 0.32, n), 1.0)
    v = np.where(active, rng.uniform(1.5, 2.5, n), rng.uniform(8.0, 9.0, n))
    return np.stack([x, v]), active


def _scan_events(cbs):
    sys_, x, v = _pendulum()
    return sys_, [hy.nt_event(x - c, cbs[k]) for k, c in enumerate(SCAN_THR)] + [hy.nt_event(v, cbs[3])]


@functools.lru_cache(maxsize=None)
def _scan_run():
    st, active = _scan_state()
    sys_, evs = _scan_events([hy.native_event_recorder() for _ in range(4)])
    a = hy.taylor_adaptive_batch(sys_, st, SCAN_N, nt_events=evs)
    hl = _HostLog()
    sys_, evs_b = _scan_events([hl.nt(k) for k in range(4)])
    b = hy.taylor_adaptive_batch(sys_, st, SCAN_N, nt_events=evs_b)
    per_step, caps = [], []
    for s in range(SCAN_STEPS):
        n0, nb0 = a.event_log_size, len(hl.rows)
        a.step()
        b.step()
        per_step.append((a.get_event_log(n0).rows, np.array(hl.rows[nb0:], dtype=float).reshape(-1, 5),
                         np.array_equal(a.state, b.state) and np.array_equal(a.time, b.time)))
        caps.append(a.event_log_capacity)
    return st, active, per_step, caps, a.event_log.rows


@pytest.mark.gpu
def test_scan_edges_on_a_large_batch():
    st, active, per_step, caps, _ = _scan_run()
    empty_block = three_rows = last_block = False
    for s, (ar, br, same) in enumerate(per_step):
        assert same, s
        assert ar.shape[0] == br.shape[0] and np.array_equal(ar[:, :5], br), s
        assert np.all(np.diff(ar[:, 0]) >= 0), s
        sysm = ar[:, 0].astype(int)
        per_lane = np.bincount(sysm, minlength=SCAN_N)
        assert np.all(per_lane[~active] == 0)
        per_block = np.add.reduceat(per_lane, np.arange(0, SCAN_N, 256))
        assert per_block.size == 258
        if ar.shape[0] != 0:
            empty_block |= bool(np.any(per_block[:-1] == 0))
            three_rows |= bool(np.any(per_lane >= 3))
            last_block |= bool(per_block[-1] > 0) and bool(np.any(sysm >= 65536 + 256))
            # (Rows from both passes of the second-level scan.)
            assert np.any(sysm < 65536) and np.any(sysm >= 65536), s
    assert empty_block and three_rows and last_block
    # The log grew past its initial capacity (the capacity after the first step, which allocated it).
    total = sum(ar.shape[0] for ar, _, _ in per_step)
    assert caps[0] >= per_step[0][0].shape[0] > 0 and total > caps[0] and caps[-1] > caps[0], (caps, total)
    print("[event log scan edges] N=%d: rows per step %s, capacities %s" % (SCAN_N, [ar.shape[0] for ar, _, _ in per_step], caps))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257])
def test_rows_of_a_system_do_not_depend_on_the_batch(n):
    st, _, _, _, big = _scan_run()
    sys_, evs = _scan_events([hy.native_event_recorder() for _ in range(4)])
    ta = hy.taylor_adaptive_batch(sys_, st[:, :n], n, nt_events=evs)
    per_step = []
    for _ in range(SCAN_STEPS):
        n0 = ta.event_log_size
        ta.step()
        per_step.append(ta.get_event_log(n0).rows)
    small = ta.event_log.rows
    ref = big[big[:, 0] < n]
    assert ref.shape[0] > 0
    # (The log is ordered by step, then by system: the rows of the first n systems of the big run, in its order.)
    assert np.array_equal(small, ref)


@pytest.mark.gpu
def test_life_cycle():
    """Test 6. propagate_until() against the host loop; accumulation across calls; the zero-copy view; counters through
    `user`; the states switch (refused on a non-empty log; headers unchanged without states); clear; a non-terminal event
    which triggers after the lane's terminal event in the same step gets no row."""
    import torch

    sys_, x, v = _pendulum()
    n = 512
    rng = np.random.RandomState(7)
    st = np.stack([rng.uniform(-0.3, 0.1, n), rng.uniform(1.0, 3.0, n)])

    def mk(nt_cbs, t_cb, with_t=True):
        return hy.taylor_adaptive_batch(sys_, st, n, nt_events=[hy.nt_event(x - 0.01, nt_cbs[0]), hy.nt_event(v, nt_cbs[1])],
                                        t_events=[hy.t_event(x, t_cb, cooldown=0.05)] if with_t else [])

    rec = [hy.native_event_recorder() for _ in range(3)]
    a = mk(rec[:2], rec[2])
    hl = _HostLog()
    b = mk([hl.nt(0), hl.nt(1)], hl.t(0))
    a.propagate_until(0.6)
    b.propagate_until(0.6)
    assert np.array_equal(a.state, b.state) and np.array_equal(a.time, b.time)
    n1 = a.event_log_size
    log = a.event_log
    br = np.array(hl.rows, dtype=float).reshape(-1, 5)
    assert n1 == br.shape[0] > 100 and np.array_equal(log.rows[:, :4], br[:, :4])
    assert np.array_equal(log.time[~log.terminal], br[~log.terminal, 4]) and np.sum(log.terminal) > 10
    # Accumulation across calls.
    a.propagate_until(1.1)
    b.propagate_until(1.1)
    br = np.array(hl.rows, dtype=float).reshape(-1, 5)
    log2 = a.event_log
    assert len(log2) == br.shape[0] > n1 and np.array_equal(log2.rows[:n1], log.rows)
    assert np.array_equal(log2.rows[:, :4], br[:, :4])
    # Counters through `user`: row counts per event.
    assert rec[0].value == np.sum(~log2.terminal & (log2.idx == 0)) and rec[1].value == np.sum(~log2.terminal & (log2.idx == 1))
    assert rec[2].value == np.sum(log2.terminal) > 0
    # The zero-copy view.
    dv = a.event_log_device
    assert dv.shape == (len(log2), 8 + 2)
    assert np.array_equal(torch.as_tensor(dv, device="cuda").cpu().numpy(), log2.rows)
    # The switch is refused while the log holds rows.
    with pytest.raises(Exception, match="only while the log is empty"):
        a.event_log_states = False
    assert a.event_log_row_size == 10
    a.clear_event_log()
    assert a.event_log_size == 0 and len(a.event_log) == 0 and a.event_log_device is None
    # Without states: the same headers, state is None.
    a2 = mk([hy.native_event_recorder(), hy.native_event_recorder()], hy.native_event_recorder())
    a2.event_log_states = False
    a2.propagate_until(0.6)
    l2 = a2.event_log
    assert l2.state is None and l2.rows.shape == (n1, 8) and np.array_equal(l2.rows, log.rows[:, :8])
    # A copy of an integrator with rows starts with an empty log and records on its own.
    c2 = a2.copy()
    assert c2.event_log_size == 0 and a2.event_log_size == n1
    # A non-terminal event after the lane's terminal event, in the same step: no row. D has the non-terminal events only;
    # A's and D's first steps start from the same state, so their roots are offsets from the same time. The case: D detects
    # x - 0.01 in a lane at an offset beyond the root of the terminal event x = 0 of A's first step.
    a3 = mk([hy.native_event_recorder(), hy.native_event_recorder()], hy.native_event_recorder())
    d = mk([hy.native_event_recorder(), hy.native_event_recorder()], None, with_t=False)
    a3.step()
    d.step()
    la, ld = a3.event_log, d.event_log
    t_root = {int(s): r for s, r in zip(la.system[la.terminal], la.root[la.terminal])}
    a_nt = {(int(s), int(i)) for s, i in zip(la.system[~la.terminal], la.idx[~la.terminal])}
    suppressed = [(int(s), float(r)) for s, i, r in zip(ld.system, ld.idx, ld.root)
                  if i == 0 and int(s) in t_root and r > t_root[int(s)]]
    assert len(suppressed) > 0
    for s, r in suppressed:
        assert (s, 0) not in a_nt
    # (... and the lane's step ends at the terminal event.)
    hs = np.array([h for _, h in a3.step_res])
    for s, _ in suppressed:
        assert hs[s] == t_root[s]
