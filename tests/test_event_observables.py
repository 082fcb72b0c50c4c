"""Event-log observables, the part which needs no GPU: the setter and its rejections, the row size, copies,
and the generated module of hy_obs_rows - compiled for gfx950, naming hy_obs_rows and nothing else of the log, without
scratch in registers mode, reading through the stage pointer in staged mode - next to an unchanged hy_dout_rows.
The values of the observables are held to cfunc of the state columns in tests/test_event_observables_gpu.py."""
import os
import subprocess

import pytest

import heyoka_amd as hy
from heyoka_amd import _lib, codegen_check, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pendulum():
    x, v = hy.make_vars("x", "v")
    return [(x, v), (v, -9.8 * hy.sin(x))], x, v


def _cpu_ta(**kw):
    """The pendulum integrator of tests/test_event_recorder.py."""
    sys_, x, v = _pendulum()
    rec = [hy.native_event_recorder() for _ in range(3)]
    ta = hy.taylor_adaptive_batch(sys_, [[0.1] * 4, [0.2] * 4], 4,
                                  nt_events=[hy.nt_event(v, rec[0]), hy.nt_event(x - 0.3, rec[1])],
                                  t_events=[hy.t_event(x + 0.3, rec[2], cooldown=0.05)], **kw)
    return ta, x, v


def _pendulum_obs(x, v):
    return [x * x + v * v, hy.sin(x), hy.time, v]


def _outer_ss(ha, **kw):
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    y1, y3 = hy.make_vars("y_1", "y_3")
    oss = hy.model.nbody(6, masses=M, Gconst=G)
    return hy.taylor_adaptive_batch(oss, None, 64, high_accuracy=ha, nt_events=[hy.nt_event(y1, hy.native_event_recorder())],
                                    t_events=[hy.t_event(y3, hy.native_event_recorder(), cooldown=0.05)], **kw), oss


def _pair_distance2(i=1, j=4):
    a = hy.make_vars(*["%s_%d" % (c, i) for c in "xyz"])
    b = hy.make_vars(*["%s_%d" % (c, j) for c in "xyz"])
    return hy.sum([(p - q) * (p - q) for p, q in zip(a, b)])


def test_row_size_round_trip_clear_and_copies():
    ta, x, v = _cpu_ta()
    assert ta.event_log_observables is None and ta.event_log_row_size == 8 + 2
    assert _lib.lib.hy_tab_get_event_log_n_observables(ta._h) == 0
    obs = _pendulum_obs(x, v)
    ta.event_log_observables = obs
    assert ta.event_log_row_size == 8 + 4 and _lib.lib.hy_tab_get_event_log_n_observables(ta._h) == 4
    assert [repr(e) for e in ta.event_log_observables] == [repr(e) for e in obs]
    log = ta.event_log
    assert len(log) == 0 and log.state is None and log.observables.shape == (0, 4) and log.rows.shape == (0, 12)
    # The states switch keeps its value and has no effect while observables are set.
    assert ta.event_log_states
    ta.event_log_states = False
    assert ta.event_log_row_size == 12 and not ta.event_log_states
    # The copy keeps the list and the switch, and shares the module.
    c = ta.copy()
    assert [repr(e) for e in c.event_log_observables] == [repr(e) for e in obs] and c.event_log_row_size == 12
    assert c.event_log_code_object(2) == ta.event_log_code_object(2) and not c.event_log_states
    # None clears: the row is what the switch says again; a copy of a cleared integrator has no list.
    ta.event_log_observables = None
    assert ta.event_log_observables is None and ta.event_log_row_size == 8 and ta.event_log.observables is None
    ta.event_log_states = True
    assert ta.event_log_row_size == 10 and ta.event_log.state.shape == (0, 2)
    assert ta.copy().event_log_observables is None and c.event_log_row_size == 12
    ta.event_log_observables = None
    with pytest.raises(ValueError, match="no event-log observables"):
        ta.event_log_code_object(2)
    # The C call: n == 0 clears, the return codes.
    lib = _lib.lib
    ex, arr = hy._handle_array([v])
    assert lib.hy_tab_set_event_log_observables(ta._h, arr, 1) == 0 and ta.event_log_row_size == 9
    assert lib.hy_tab_set_event_log_observables(ta._h, None, 0) == 0 and ta.event_log_row_size == 10
    assert lib.hy_tab_set_event_log_observables(ta._h, None, 2) != 0 and "null" in _lib.last_error()


def test_rejections_and_their_messages(monkeypatch):
    ta, x, v = _cpu_ta()
    with pytest.raises(ValueError, match="The list of observables of the event log is empty"):
        ta.event_log_observables = []
    q = hy.make_vars("q")
    q = q[0] if isinstance(q, (list, tuple)) else q
    with pytest.raises(ValueError, match="The observable 1 of the event log uses the variable 'q', which is not a state variable"):
        ta.event_log_observables = [x, q * v]
    with pytest.raises(ValueError, match=r"An observable of the event log uses par\[2\], but the integrator has 0 parameter"):
        ta.event_log_observables = [x * hy.par[2]]
    assert ta.event_log_observables is None and ta.event_log_row_size == 10
    # An integrator without recorders: the message family of event_log_code_object().
    sys_, x2, v2 = _pendulum()
    plain = hy.taylor_adaptive_batch(sys_, None, 4, nt_events=[hy.nt_event(v2, hy.native_event_counter())])
    with pytest.raises(ValueError, match="no recording event callbacks"):
        plain.event_log_observables = [x2]
    with pytest.raises(ValueError, match="no recording event callbacks"):
        plain.event_log_observables = None
    with pytest.raises(ValueError, match="no recording event callbacks"):
        plain.event_log_code_object(2)
    # The switch of the way of holding the samples.
    monkeypatch.setenv("HEYOKA_AMD_EVENT_OBS", "lds")
    with pytest.raises(ValueError, match="Invalid value 'lds' of HEYOKA_AMD_EVENT_OBS: 'registers' or 'staged'"):
        ta.event_log_observables = [x]
    with pytest.raises(ValueError, match="HEYOKA_AMD_EVENT_OBS"):
        hy.event_observables_source(sys_, [x2])
    monkeypatch.setenv("HEYOKA_AMD_EVENT_OBS", "registers")
    ta.event_log_observables = [x]
    assert ta.event_log_row_size == 9


def _check_module(ta, n_reads, staged=False):
    src, co = ta.event_log_source(2), ta.event_log_code_object(2)
    assert co[:4] == b"\x7fELF" and b"gfx950" in co
    assert b"hy_obs_rows" in co
    for k in (b"hy_dout_rows", b"hy_evr_", b"hy_detect_events", b"hy_taylor"):
        assert k not in co, k
    assert "hy_obs_rows(const hy_drow_args a)" in src and "hy_dout_rows" not in src.split("struct hy_drow_args")[1]
    assert "samples of the %d state row(s) the observables read (%s)" % (n_reads, "staged" if staged else "registers") in src
    assert ("a.stage" in src.split("hy_obs_rows(const")[1]) == staged
    res = codegen_check.kernel_resources(co, kernel="hy_obs_rows")
    print("[hy_obs_rows] %d rows read, %s: %s" % (n_reads, "staged" if staged else "registers", res))
    return src, res


@pytest.mark.parametrize("ha", [False, True])
def test_pendulum_module(ha):
    ta, x, v = _cpu_ta(high_accuracy=ha)
    ta.event_log_observables = _pendulum_obs(x, v)
    src, res = _check_module(ta, 2)
    assert res["vgpr_spill"] == 0 and res["scratch_bytes_per_lane"] == 0
    sys_ = _pendulum()[0]
    assert src == hy.event_observables_source(sys_, _pendulum_obs(x, v), order=ta.order, high_accuracy=ha)
    assert ("comp = (t - res) - y;" in src) == ha
    # (Only the rows read are sampled: an observable of v alone never touches the coefficients of x.)
    ta.event_log_observables = [v]
    src = ta.event_log_source(2)
    assert "((u64)1u * 21u) * N + s" in src and "((u64)0u * 21u) * N + s" not in src


@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("kw", [{}, {"cluster_kernel": "v2"}], ids=["v5", "v2"])
def test_outer_solar_system_modules(kw, ha):
    ta, oss = _outer_ss(ha, **kw)
    assert ("v2" in ta.hip_source_mode) == bool(kw)
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    for obs, n_reads in (([_pair_distance2()], 6), ([hy.model.nbody_energy(6, masses=M, Gconst=G)], 36)):
        ta.event_log_observables = obs
        src, res = _check_module(ta, n_reads)
        assert res["vgpr_spill"] == 0 and res["scratch_bytes_per_lane"] == 0
        compact = "hy_rk_c" in ta.event_log_source(1)
        assert src == hy.event_observables_source(oss, obs, order=ta.order, high_accuracy=ha, compact_tc=compact)
        if compact and n_reads == 6:
            # Positions only: rows defined by their velocities - the parents' coefficients, the rows' own order 0.
            assert src.count("const double x0_") == 6 and "double rv" not in src


def test_staged_mode_reads_through_the_stage_pointer(monkeypatch):
    ta, oss = _outer_ss(True)
    M, G = configs.OUTER_SS_MASSES, configs.OUTER_SS_G
    en = [hy.model.nbody_energy(6, masses=M, Gconst=G)]
    ta.event_log_observables = en
    reg = ta.event_log_source(2)
    ta.event_log_observables = None
    monkeypatch.setenv("HEYOKA_AMD_EVENT_OBS", "staged")
    ta.event_log_observables = en
    src, _ = _check_module(ta, 36, staged=True)
    assert src != reg and "double *stg = a.stage + r;" in src and "((const volatile double *)stg)[(u64)35u * a.n_max]" in src
    assert "stg[(u64)36u" not in src
    # Above the register budget the staging buffer is the default.
    monkeypatch.delenv("HEYOKA_AMD_EVENT_OBS")
    vs = hy.make_vars(*["q%d" % i for i in range(70)])
    big = [(q, -q) for q in vs]
    assert "a.stage" not in hy.event_observables_source(big, [hy.sum(vs[:64])]).split("hy_obs_rows(const")[1]
    assert "a.stage" in hy.event_observables_source(big, [hy.sum(vs[:65])]).split("hy_obs_rows(const")[1]


def test_dout_rows_source_is_unchanged_by_setting_and_clearing():
    """hy_dout_rows before the observables are set, while they are set and after they are cleared: one text. (The text is
    not reachable on the commit before this feature - only its code object is -, so there is no hash of it to pin.)"""
    for ta, x, v in (_cpu_ta(), _cpu_ta(high_accuracy=True)):
        before, co = ta.event_log_source(1), ta.event_log_code_object(1)
        assert "hy_dout_rows" in before and "hy_obs_rows" not in before
        ta.event_log_observables = _pendulum_obs(x, v)
        assert ta.event_log_source(1) == before and ta.event_log_code_object(1) == co
        ta.event_log_observables = None
        assert ta.event_log_source(1) == before and ta.event_log_code_object(1) == co
        assert ta.event_log_code_object(0) == _cpu_ta()[0].event_log_code_object(0)


def test_dout_rows_takes_the_extended_block_and_does_not_read_its_new_fields():
    """What did change in the text of hy_dout_rows: the argument block it shares with hy_obs_rows ends with the two new
    fields. Its kernel never reads them, and the blocks of the two kernels are one text."""
    ta, x, v = _cpu_ta()
    ta.event_log_observables = [x]
    block = "struct hy_drow_args {\n    double *rows;\n    const double *tc;\n    const double *state;\n    const u64 *n_rows;\n" \
            "    u64 n_max;\n    u64 N;\n    unsigned row_doubles, pad;\n    const double *pars;\n    double *stage;\n};\n"
    for which in (1, 2):
        assert ta.event_log_source(which).count(block) == 1 and ta.event_log_source(which).count("struct hy_drow_args") == 1
    body = ta.event_log_source(1).split("hy_dout_rows(const hy_drow_args a)")[1]
    assert "a.pars" not in body and "a.stage" not in body and "a.tc" in body and "a.state" in body


EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_event_observables")


def _build_cpp():
    """tests/cpp/test_event_observables.cpp, compiled the way tests/test_event_recorder.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_event_observables.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_event_observables_host_half():
    out = subprocess.run([_build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_cpp_event_observables_on_gpu():
    out = subprocess.run([_build_cpp(), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GPU OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
