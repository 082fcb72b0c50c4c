"""Grid statistics: propagate_grid() folds its observables over the grid, per system. Host half: the modules
without statistics are, byte for byte, those of the commit before the feature; the generated module which folds (hiprtc
cross-compiles without a GPU) and its resources in both ways of holding the samples; the checks of the list of statistics in
every front end; the C ABI; the module cache; the C++ program written against <heyoka/heyoka.hpp>. The numbers are checked in
tests/test_grid_statistics_gpu.py."""
import copy
import ctypes
import hashlib
import os
import re
import subprocess

import pytest

import heyoka_amd as hy
from heyoka_amd import _lib, codegen_check

from test_grid_observables import CASES, energy_case, pendulum_case, rows_loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_grid_statistics")
ALL = ["min", "max", "t_min", "t_max", "sum", "last", "count"]

# sha256 of hy.grid_observables_source(case, order=20, high_accuracy=ha) at the commit before grid statistics.
PARENT_SHA256 = {
    ("pendulum_case", False): "a7b03181ee822bcf7323f0510505d7b4d384fb4558dc5290d73f827dcc48f20c",
    ("pendulum_case", True): "ebcea9117760e9968faeccff99f82efed433a01de2da249886cb13250f1f5356",
    ("energy_case", False): "d031bebbb7258149da8c5e95de764bc045ec12d886505f5aedde77e535e61da2",
    ("energy_case", True): "95076ba5197617e4f7e60fce5334404006686481cae3c9f3c36e3b0d79b6dfed",
    ("distance_case", False): "31e55f75f9c6e0634a5c47dd1087d94e6db9ed4659c397029ace1d5daf2a7c4f",
    ("distance_case", True): "5661b7f68cd9f4d9bbcb99837a7e28fb038eb386c7c541e063d7e082511b9c32",
}


def stats_of(case):
    """All seven, and the three of the energy error of the benchmark protocol for the 36-row energy."""
    return ["min", "max", "t_max"] if case is energy_case else ALL


def kernel(src, name):
    return src.split("%s(const hy_grid_args a)" % name)[1].split('extern "C"')[0]


@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_sources_without_statistics_are_those_of_the_parent_commit(case, ha, monkeypatch):
    monkeypatch.delenv("HEYOKA_AMD_GRID_OBS", raising=False)
    sys_, obs, _, _ = case()
    src = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha)
    assert hashlib.sha256(src.encode()).hexdigest() == PARENT_SHA256[(case.__name__, ha)]
    assert "HY_NSLOT" not in src and "shadowed" not in src


@pytest.mark.parametrize("mode", ["registers", "staged"])
@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_source_folds_and_compiles_without_scratch(case, ha, mode, monkeypatch):
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", mode)
    sys_, obs, n_rows, dim = case()
    stats = stats_of(case)
    src = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha, statistics=stats)
    plain = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha)
    for k in ("hy_grid_post", "hy_grid_obs0", "hy_grid_unsample", "hy_until_post", "hy_indep_override"):
        assert 'extern "C" __global__ void __launch_bounds__(256) %s(' % k in src
    assert "#define HY_HA %d" % int(ha) in src and "#define HY_DIM %du" % dim in src and "#define HY_NOUT 1u" in src
    assert "#define HY_NSLOT %du" % len(stats) in src and "__shared__" not in src
    assert len(rows_loaded(src)) == n_rows
    post, un, obs0 = kernel(src, "hy_grid_post"), kernel(src, "hy_grid_unsample"), kernel(src, "hy_grid_obs0")
    sec = src.split("void hy_obs_section(")[1].split('extern "C"')[0]
    # Nothing is stored per grid point: no store indexed by g anywhere, no NaN fill, and the same row loop as without.
    assert not re.search(r"out[0p]?\[\(\(u64\)g", src) and "(u64)g * HY_NOUT" not in src
    assert "__builtin_nan" not in un and "g < g1" not in un
    assert ("stg[(u64)v * N] = res;" in post) == (mode == "staged") and ("xs[j] = res;" in post) == (mode == "registers")
    rows = lambda s: s.split("const double *tcb = tc0;")[1].split("hy_obs_section(a, i, N")[0]  # noqa: E731
    assert rows(post) == rows(kernel(plain, "hy_grid_post"))
    # The shadow copy ahead of the first merge of a sweep, and its way back.
    assert "if (!shadowed) {" in post and "out0[(u64)(HY_NSLOT + s) * N] = out0[(u64)s * N];" in post
    assert post.index("if (!shadowed) {") < post.index("const double *tcb = tc0;")
    assert "if (a.gidx_prev[i] < a.gidx[i]) {" in un and "a.out[(u64)s * N + i] = a.out[(u64)(HY_NSLOT + s) * N + i];" in un
    # The merge: the comparisons of the table, the sum as one rounded addition of an opaque value.
    assert 'asm volatile("" : "+v"(y0));' in sec
    assert "if (y0 < m || m != m) {" in sec and "if (y0 > m || m != m) {" in sec
    assert ("__dadd_rn(outp[(u64)4u * N], y0)" in sec) == ("sum" in stats)
    assert "if (g == 0u) {" in sec and "hy_obs_section(a, i, N, a.out + i, 0u, a.grid[i]" in obs0
    co = hy.hiprtc_compile(src)
    assert co[:4] == b"\x7fELF"
    for k in ("hy_grid_post", "hy_grid_obs0"):
        res = codegen_check.kernel_resources(co, kernel=k)
        assert res is not None
        print(case.__name__, ha, mode, k, res)
        assert res["scratch_bytes_per_lane"] == 0 and res["vgpr_spill"] == 0 and res["lds_bytes"] == 0, (k, res)
        # (Staged: a pair of SGPRs may be parked in a VGPR lane, as without statistics.)
        assert res["sgpr_spill"] == 0 or mode == "staged", (k, res)


def test_hidden_slots_and_the_order_of_the_list():
    sys_, obs, _, _ = pendulum_case()
    src = hy.grid_observables_source(sys_, obs, statistics=["t_max", "count", "t_min"])
    sec = src.split("void hy_obs_section(")[1].split('extern "C"')[0]
    # Slots 0..2 are the output in the order given; the extrema behind t_min / t_max live in the hidden slots 3 and 4.
    assert "#define HY_NSLOT 5u" in src
    assert "{ const double m = outp[(u64)3u * N]; if (y0 < m || m != m) { outp[(u64)3u * N] = y0; outp[(u64)2u * N] = t_hi; } }" in sec
    assert "{ const double m = outp[(u64)4u * N]; if (y0 > m || m != m) { outp[(u64)4u * N] = y0; outp[(u64)0u * N] = t_hi; } }" in sec
    assert "outp[(u64)1u * N] = outp[(u64)1u * N] + 1.0;" in sec and "__dadd_rn" not in sec


def test_the_switch_over_still_follows_the_number_of_rows(monkeypatch):
    monkeypatch.delenv("HEYOKA_AMD_GRID_OBS", raising=False)
    sys_ = hy.model.nbody(11)
    vs = hy._to_sys(sys_).vars
    assert "a.stage" not in hy.grid_observables_source(sys_, [hy.sum(vs[:64])], statistics=ALL)
    src = hy.grid_observables_source(sys_, [hy.sum(vs)], statistics=ALL)
    assert "double *stg = a.stage + i;" in src and len(rows_loaded(src)) == 66 and "#define HY_NSLOT 7u" in src


def test_checks_of_the_statistics_in_every_front_end():
    x, v, w = hy.make_vars("x", "v", "w")
    sys_ = [(x, v), (v, -hy.par[0] * x)]
    ta = hy.taylor_adaptive_batch(sys_, None, 4)
    obs = [x * v]
    bad = [
        (obs, [], r"The list of statistics of propagate_grid\(\) is empty"),
        (obs, ["min", "median"], r"The statistic 'median' of propagate_grid\(\) is unknown"),
        (obs, ["sum", "min", "sum"], r"The statistic 'sum' of propagate_grid\(\) is named twice"),
        (None, ["min"], r"The statistics of propagate_grid\(\) need a list of observables"),
        # The checks of the observables keep their messages.
        ([x * v, w + x], ALL, "The observable 1 of propagate_grid\\(\\) uses the variable 'w', which is not a state variable"),
        ([hy.par[1] * x], ALL, r"An observable of propagate_grid\(\) uses par\[1\], but the integrator has 1 parameter\(s\)"),
        ([], ALL, r"The list of observables of propagate_grid\(\) is empty"),
    ]
    for o, st, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid([0.0, 1.0], observables=o, statistics=st)
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid([0.0, 1.0], observables=o, statistics=st, callback=lambda t: True)
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid_device([0.0, 1.0], 8, observables=o, statistics=st)
        with pytest.raises(ValueError, match=msg):
            ta.grid_observables_module(o, statistics=st)
        if "parameter" not in msg:  # (without an integrator there is no parameter array to check against)
            with pytest.raises(ValueError, match=msg):
                hy.grid_observables_source(sys_, o, statistics=st)
    assert "hy_grid_post" in ta.grid_observables_module(obs, statistics=ALL)[0]


def test_c_abi_round_trip():
    lib = _lib.lib
    sys_, obs, _, _ = pendulum_case()
    s = hy._to_sys(sys_)
    arr = (ctypes.c_void_p * 1)(obs[0]._h)
    null = (ctypes.c_void_p * 1)(None)
    codes = (ctypes.c_int * 7)(*range(7))
    err = lambda: lib.hy_last_error().decode()  # noqa: E731
    p = lib.hy_grid_stats_source(s._h, arr, 1, codes, 7, 20, 1)
    assert p
    assert _lib.take_str(p) == hy.grid_observables_source(sys_, obs, order=20, high_accuracy=True, statistics=ALL)
    assert not lib.hy_grid_stats_source(None, arr, 1, codes, 7, 20, 0)
    assert err() == "hy_grid_stats_source(): the system handle is null"
    assert not lib.hy_grid_stats_source(s._h, null, 1, codes, 7, 20, 0)
    assert err() == "hy_grid_stats_source(): the observable 0 is a null expression"
    assert not lib.hy_grid_stats_source(s._h, arr, 1, None, 7, 20, 0)
    assert err() == "hy_grid_stats_source(): the array of statistics is null"
    assert not lib.hy_grid_stats_source(s._h, arr, 1, (ctypes.c_int * 2)(0, 7), 2, 20, 0)
    assert err() == "The statistic code 7 of propagate_grid() is unknown"
    assert not lib.hy_grid_stats_source(s._h, arr, 1, (ctypes.c_int * 2)(-1, 0), 2, 20, 0)
    assert err() == "The statistic code -1 of propagate_grid() is unknown"
    assert not lib.hy_grid_stats_source(s._h, arr, 1, (ctypes.c_int * 2)(5, 5), 2, 20, 0)
    assert err() == "The statistic 'last' of propagate_grid() is named twice"
    assert not lib.hy_grid_stats_source(s._h, arr, 1, codes, 0, 20, 0)
    assert err() == "The list of statistics of propagate_grid() is empty"
    ta = hy.taylor_adaptive_batch(sys_, None, 4, pars=[[0.0] * 4, [1.0] * 4])
    out = (ctypes.c_double * 28)()
    grid = (ctypes.c_double * 8)(*([0.0] * 4 + [1.0] * 4))
    bad = (ctypes.c_int * 1)(9)
    invalid = lib.hy_tab_propagate_grid_stats(None, grid, 2, 0, None, 0, None, 0, arr, 1, codes, 7, out)
    assert invalid != 0 and err() == "hy_tab_propagate_grid_stats(): the integrator handle is null"
    assert lib.hy_tab_propagate_grid_stats(ta._h, grid, 2, 0, None, 0, None, 0, null, 1, codes, 7, out) == invalid
    assert err() == "hy_tab_propagate_grid_stats(): the observable 0 is a null expression"
    assert lib.hy_tab_propagate_grid_stats(ta._h, grid, 2, 0, None, 0, None, 0, arr, 1, None, 7, out) == invalid
    assert err() == "hy_tab_propagate_grid_stats(): the array of statistics is null"
    assert lib.hy_tab_propagate_grid_stats(ta._h, grid, 2, 0, None, 0, None, 0, arr, 1, bad, 1, out) == invalid
    assert err() == "The statistic code 9 of propagate_grid() is unknown"
    # (Every function names itself.)
    assert lib.hy_tab_propagate_grid_stats_device(None, grid, 2, 0, 0, None, 0, arr, 1, codes, 7, out) == invalid
    assert err() == "hy_tab_propagate_grid_stats_device(): the integrator handle is null"
    assert lib.hy_tab_propagate_grid_stats_device(ta._h, grid, 2, 0, 0, None, 0, null, 1, codes, 7, out) == invalid
    assert err() == "hy_tab_propagate_grid_stats_device(): the observable 0 is a null expression"
    assert lib.hy_tab_propagate_grid_stats_device(ta._h, grid, 2, 0, 0, None, 0, arr, 1, None, 1, out) == invalid
    assert err() == "hy_tab_propagate_grid_stats_device(): the array of statistics is null"
    assert lib.hy_tab_propagate_grid_stats_device(ta._h, grid, 2, 0, 0, None, 0, arr, 1, bad, 1, out) == invalid
    assert err() == "The statistic code 9 of propagate_grid() is unknown"
    assert lib.hy_tab_propagate_grid_stats_device(ta._h, grid, 2, 0, 0, None, 0, arr, 1, codes, 7, None) == invalid
    assert err() == "hy_tab_propagate_grid_stats_device(): the device output pointer is null"
    assert lib.hy_tab_grid_stats_module(None, arr, 1, codes, 7, None, None, None) == invalid
    assert err() == "hy_tab_grid_stats_module(): the integrator handle is null"
    assert lib.hy_tab_grid_stats_module(ta._h, null, 1, codes, 7, None, None, None) == invalid
    assert err() == "hy_tab_grid_stats_module(): the observable 0 is a null expression"
    assert lib.hy_tab_grid_stats_module(ta._h, arr, 1, None, 2, None, None, None) == invalid
    assert err() == "hy_tab_grid_stats_module(): the array of statistics is null"
    assert lib.hy_tab_grid_stats_module(ta._h, arr, 1, bad, 1, None, None, None) == invalid
    assert lib.hy_tab_grid_stats_module(ta._h, arr, 1, codes, 7, None, None, None) == 0
    # The constants of the header are the positions in the list of names.
    hdr = open(os.path.join(ROOT, "include", "heyoka_amd.h")).read()
    for k, name in enumerate(ALL):
        assert "#define HY_GRID_STAT_%s %d\n" % (name.upper(), k) in hdr
    assert list(hy.GRID_STATISTICS) == ALL


def test_module_cache_and_sources_untouched():
    """One module per (observables, statistics), kept in the integrator; a copy regenerates the same text; neither the
    stepper's source nor the event-detection source nor the module of the observables alone changes."""
    sys_, obs, _, _ = pendulum_case()
    x, v = hy._to_sys(sys_).vars
    ta = hy.taylor_adaptive_batch(sys_, None, 8, nt_events=[hy.nt_event(v, hy.native_event_counter())], high_accuracy=True)
    ed = lambda: _lib.take_str(_lib.lib.hy_event_detection_source(ta.order, 0, 1))  # noqa: E731
    stepper, detection = ta.hip_source, ed()
    plain = ta.grid_observables_module(obs)
    src, co = ta.grid_observables_module(obs, statistics=ALL)
    assert co[:4] == b"\x7fELF" and src != plain[0] and co != plain[1]
    assert src == hy.grid_observables_source(sys_, obs, order=ta.order, high_accuracy=True, statistics=ALL)
    assert ta.grid_observables_module(list(obs), statistics=list(ALL)) == (src, co)
    assert ta.grid_observables_module(obs) == plain
    assert ta.hip_source == stepper and ed() == detection
    tb = copy.deepcopy(ta)
    assert tb.grid_observables_module(obs, statistics=ALL) == (src, co)
    assert tb.hip_source == stepper
    # Another list of statistics - another order too - is another module, and so is another list of observables.
    assert ta.grid_observables_module(obs, statistics=["min", "max"])[0] != src
    assert ta.grid_observables_module(obs, statistics=ALL[::-1])[0] != src
    assert ta.grid_observables_module([x * v], statistics=ALL)[0] != src


def build_cpp():
    """tests/cpp/test_grid_statistics.cpp, compiled the way tests/test_grid_observables.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_grid_statistics.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_grid_statistics_host_half():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
