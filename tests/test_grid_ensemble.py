"""Ensemble statistics: propagate_grid() folds its observables across the systems per grid point, exactly.
Host half: the accumulators - host add, merge and finish - against a reference in rational arithmetic; the generated module
which merges (hiprtc cross-compiles without a GPU) and its resources; the refusals in every front end; the C++ program. The
numbers of the kernels are checked in tests/test_grid_ensemble_gpu.py, which uses ref_fold() from here."""
import ctypes
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import _lib, codegen_check

from test_grid_observables import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_grid_ensemble")
ALL = ["count", "min", "max", "sum", "sum_sq", "mean"]
INF, NAN = float("inf"), float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit for bit where neither is NaN (so -0.0 is not +0.0), and the same NaN pattern."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---- the reference: the table of the design, in rational arithmetic ----
def total_order_key(v):
    """-inf < ... < -0.0 < +0.0 < ... < +inf."""
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | (1 << 63))


def exact_sum(vals):
    """The exact sum of non-NaN doubles, rounded once to nearest-even, with the rules of the table for zero, overflow and
    infinities."""
    pinf, ninf = any(v == INF for v in vals), any(v == -INF for v in vals)
    if pinf or ninf:
        return NAN if pinf and ninf else (INF if pinf else -INF)
    s = sum((Fraction(v) for v in vals), Fraction(0))
    if s == 0:
        return 0.0
    try:
        return float(s)  # (int / int: correctly rounded, OverflowError when the rounded result is beyond the largest double)
    except OverflowError:
        return INF if s > 0 else -INF


def ref_stats(values, stats):
    """The statistics of the values which are not NaN, in the order of stats."""
    V = [float(v) for v in np.asarray(values, dtype=float).reshape(-1) if v == v]
    with np.errstate(over="ignore", under="ignore"):
        Q = [float(np.float64(v) * np.float64(v)) for v in V]  # one rounded multiplication, inf on overflow
    r = dict(count=float(len(V)), min=min(V, key=total_order_key) if V else NAN, max=max(V, key=total_order_key) if V else NAN,
             sum=exact_sum(V), sum_sq=exact_sum(Q))
    with np.errstate(all="ignore"):
        r["mean"] = float(np.float64(r["sum"]) / np.float64(r["count"])) if V else NAN
    return [r[s] for s in stats]


def ref_fold(y, stats):
    """y[point, observable, lane] -> [point, observable, statistic]."""
    n_grid, n_obs, _ = y.shape
    return np.array([[ref_stats(y[g, o], stats) for o in range(n_obs)] for g in range(n_grid)]).reshape(n_grid, n_obs, len(stats))


def host_fold(values, stats, parts=1, seed=0):
    """The values dealt over `parts` sets of accumulators by the host twin of the kernel, merged into the first."""
    accs = [hy.ensemble_accumulators(1, 1, stats) for _ in range(parts)]
    where = np.random.RandomState(seed).randint(0, parts, len(values))
    for v, k in zip(values, where):
        accs[k].add(0, 0, v)
    for a in accs[1:]:
        accs[0].merge(a)
    return accs[0]


def random_doubles(n, seed):
    """Finite doubles, NaN and infinities left out, uniform over the bit patterns: every exponent and both signs."""
    b = np.random.RandomState(seed).randint(0, 2**63, size=2 * n, dtype=np.int64).astype(np.uint64)
    b |= np.random.RandomState(seed + 1).randint(0, 2, size=2 * n).astype(np.uint64) << np.uint64(63)
    v = b.view(np.float64)
    return v[np.isfinite(v)][:n]


TINY = 2.0**-1074
ADVERSARIAL = {
    "random over the whole exponent range": random_doubles(300, 1),
    "cancellation": [1e308, 1.0, -1e308],
    "a thousand times the smallest subnormal": [TINY] * 1000,
    "zeros of both signs": [0.0, -0.0, -0.0],
    "negative zeros only": [-0.0, -0.0],
    "the exact sum overflows, no partial sum does": [1.7e308] * 3,
    "the same, negative": [-1.7e308] * 3,
    "overflow which a later value takes back": [1.7e308, 1.7e308, -1.7e308, 5.0],
    "+inf": [1.0, INF, -3.0],
    "-inf": [-INF, 2.0, -INF],
    "both infinities": [INF, 1.0, -INF],
    "NaN entries are skipped": [NAN, 1.5, NAN, -0.25],
    "NaN only": [NAN, NAN],
    "empty": [],
    "a tie rounds to even, down": [1.0, 2.0**-53],
    "a tie rounds to even, up": [1.0 + 2.0**-52, 2.0**-53],
    "a tie broken by a sticky bit far below": [1.0, 2.0**-53, TINY],
    "a tie broken downwards by a negative sticky bit": [1.0 + 2.0**-52, 2.0**-53, -TINY],
    "rounding carries into the next binade": [2.0 - 2.0**-52, 2.0**-53],
    "rounding carries into infinity": [1.7976931348623157e308, 2.0**970],
    "just below that": [1.7976931348623157e308, 2.0**970, -TINY],
    "subnormal result of a cancellation": [1.0, -1.0, 3 * TINY, -TINY],
    "squares which overflow and underflow": [1e200, -1e200, 1e-200, -1e-200, 3.0],
    "squares around the subnormal threshold": [1.5e-154, 2.0**-537, 2.0**-538, 1.4916681462400413e-154],
    "negative sum": [-1.0, -2.0**-60, 0.5],
}


@pytest.mark.parametrize("name", list(ADVERSARIAL))
@pytest.mark.parametrize("parts", [1, 2, 7])
def test_host_add_merge_finish_against_rational_arithmetic(name, parts):
    vals = np.asarray(ADVERSARIAL[name], dtype=float)
    exp = ref_stats(vals, ALL)
    one = host_fold(vals, ALL)
    acc = host_fold(vals, ALL, parts, seed=len(vals))
    got = acc.values
    print(name, parts, got.reshape(-1), exp)
    assert got.shape == (1, 1, len(ALL)) and same(got.reshape(-1), exp)
    # Any partition of the values merges to the words of the single set.
    assert acc.raw.dtype == np.uint64 and np.array_equal(acc.raw, one.raw)
    rev = host_fold(vals[::-1], ALL)
    assert np.array_equal(rev.raw, one.raw)


def test_the_reference_itself_on_cases_known_by_hand():
    assert ref_stats([1e308, 1.0, -1e308], ["sum"]) == [1.0]
    assert ref_stats([1.7e308] * 3, ["sum", "sum_sq"]) == [INF, INF]
    assert ref_stats([TINY] * 1000, ["sum"]) == [1000 * TINY]
    assert same(ref_stats([-0.0, -0.0], ["sum", "min", "max"]), [0.0, -0.0, -0.0])
    assert same(ref_stats([0.0, -0.0], ["min", "max"]), [-0.0, 0.0])
    assert ref_stats([1.0, 2.0**-53], ["sum"]) == [1.0] and ref_stats([1.0, 2.0**-53, TINY], ["sum"]) == [1.0 + 2.0**-52]
    assert same(ref_stats([], ALL), [0.0, NAN, NAN, 0.0, 0.0, NAN])
    assert ref_stats([1e-200], ["sum_sq"]) == [0.0]


def test_min_max_follow_the_key_order():
    vals = [3.0, -0.0, 0.0, -TINY, TINY, -INF, INF, -2.5, NAN]
    for k in range(1, len(vals) + 1):
        sub = vals[:k]
        got = host_fold(sub, ["min", "max"]).values.reshape(-1)
        assert same(got, ref_stats(sub, ["min", "max"])), sub
    assert same(host_fold([0.0, -0.0], ["min", "max"]).values.reshape(-1), [-0.0, 0.0])
    assert same(host_fold([-0.0, 0.0], ["max", "min"]).values.reshape(-1), [0.0, -0.0])
    srt = sorted([v for v in vals if v == v], key=total_order_key)
    assert same(srt, [-INF, -2.5, -TINY, -0.0, 0.0, TINY, 3.0, INF])


def test_record_holds_only_what_the_list_needs():
    words = lambda st: hy.ensemble_accumulators(3, 2, st).raw.size // 6  # noqa: E731
    assert words(["count"]) == 1 and words(["min"]) == 1 and words(["max", "min", "count"]) == 3
    assert words(["sum"]) == 68 and words(["mean"]) == 69 and words(["mean", "count", "sum"]) == 69
    assert words(["sum_sq"]) == 68 and words(ALL) == 3 + 2 * 68
    # The order of the list is the order of the values, not of the record.
    a, b = hy.ensemble_accumulators(1, 1, ["max", "count"]), hy.ensemble_accumulators(1, 1, ["count", "max"])
    for acc in (a, b):
        acc.add(0, 0, 2.0).add(0, 0, -1.0)
    assert np.array_equal(a.raw, b.raw) and list(a.values.reshape(-1)) == [2.0, 2.0] and list(b.values.reshape(-1)) == [2.0, 2.0]
    with pytest.raises(ValueError, match="different shapes or statistics"):
        a.merge(b)
    # Records are per (point, observable).
    c = hy.ensemble_accumulators(2, 2, ["sum"])
    c.add(1, 0, 4.0).add(0, 1, -1.0)
    assert np.array_equal(c.values[:, :, 0], [[0.0, -1.0], [4.0, 0.0]])


def kernel(src, name):
    return src.split("%s(const hy_grid_args a)" % name)[1].split('extern "C"')[0]


HEADLINE = ["count", "mean", "min", "max", "sum_sq"]


@pytest.mark.parametrize("agg", ["aggregate", "peratomic"])
@pytest.mark.parametrize("mode", ["registers", "staged"])
@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_source_merges_and_compiles_without_scratch(case, ha, mode, agg, monkeypatch):
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", mode)
    monkeypatch.setenv("HEYOKA_AMD_GRID_ENS", agg)
    sys_, obs, n_rows, dim = case()
    src = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha, ensemble_statistics=HEADLINE)
    plain = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha)
    for k in ("hy_grid_post", "hy_grid_obs0", "hy_until_post", "hy_indep_override"):
        assert 'extern "C" __global__ void __launch_bounds__(256) %s(' % k in src
    assert "hy_grid_unsample" not in src and "__shared__" not in src
    assert "#define HY_ENS_WORDS 139u" in src and "#define HY_ENS_AGG %d" % (agg == "aggregate") in src
    post, obs0 = kernel(src, "hy_grid_post"), kernel(src, "hy_grid_obs0")
    sec = src.split("void hy_obs_section(")[1].split('extern "C"')[0]
    # The same row loop as without, the opaque value, the merge into record (g, o) behind the start of the output.
    rows = lambda s: s.split("const double *tcb = tc0;")[1].split("hy_obs_section(a, i, N")[0]  # noqa: E731
    assert rows(post) == rows(kernel(plain, "hy_grid_post"))
    assert 'asm volatile("" : "+v"(y0));' in sec
    assert "hy_ens_merge((u64 *)outp + ((u64)g * HY_NOUT + 0u) * HY_ENS_WORDS, y0);" in sec
    assert "hy_obs_section(a, i, N, a.out, g, tg.hi" in post and "hy_obs_section(a, i, N, a.out, 0u, a.grid[i]" in obs0
    # No floating-point atomics, and the split of a double is the text the host compiles.
    assert "atomicAdd(" in src and "unsafeAtomicAdd" not in src and "atomicAdd((double" not in src and "atomicAdd((float" not in src
    assert "HY_ENS_FN unsigned hy_ens_split(const u64 bits" in src and "HY_ENS_FN u64 hy_ens_key(const u64 bits)" in src
    co = hy.hiprtc_compile(src)
    assert co[:4] == b"\x7fELF"
    for k in ("hy_grid_post", "hy_grid_obs0"):
        res = codegen_check.kernel_resources(co, kernel=k)
        assert res is not None
        print(case.__name__, ha, mode, agg, k, res)
        assert res["scratch_bytes_per_lane"] == 0 and res["vgpr_spill"] == 0 and res["lds_bytes"] == 0, (k, res)
        # (Staged: a pair of SGPRs may be parked in a VGPR lane, as without the statistics.)
        assert res["sgpr_spill"] == 0 or mode == "staged", (k, res)


def test_the_existing_variants_do_not_change_with_the_switch(monkeypatch):
    sys_, obs, _, _ = CASES[0]()
    monkeypatch.delenv("HEYOKA_AMD_GRID_ENS", raising=False)
    a = (hy.grid_observables_source(sys_, obs), hy.grid_observables_source(sys_, obs, statistics=["min", "sum"]))
    monkeypatch.setenv("HEYOKA_AMD_GRID_ENS", "peratomic")
    b = (hy.grid_observables_source(sys_, obs), hy.grid_observables_source(sys_, obs, statistics=["min", "sum"]))
    assert a == b and "hy_ens" not in a[0] and "hy_ens" not in a[1]
    monkeypatch.setenv("HEYOKA_AMD_GRID_ENS", "sometimes")
    with pytest.raises(ValueError, match="Invalid value 'sometimes' of HEYOKA_AMD_GRID_ENS: 'aggregate' or 'peratomic'"):
        hy.grid_observables_source(sys_, obs, ensemble_statistics=["count"])


def test_observables_of_the_parameters_alone_compile():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -x)]
    src = hy.grid_observables_source(sys_, [hy.par[0], hy.par[0] * hy.par[1]], ensemble_statistics=ALL)
    assert "#define HY_NROWS 0u" in src and hy.hiprtc_compile(src)[:4] == b"\x7fELF"


def test_refusals_in_every_front_end():
    x, v, w = hy.make_vars("x", "v", "w")
    sys_ = [(x, v), (v, -hy.par[0] * x)]
    ta = hy.taylor_adaptive_batch(sys_, None, 4)
    obs = [x * v]
    bad = [
        (obs, None, [], r"The list of ensemble statistics of propagate_grid\(\) is empty"),
        (obs, None, ["min", "median"], r"The ensemble statistic 'median' of propagate_grid\(\) is unknown"),
        (obs, None, ["sum", "min", "sum"], r"The ensemble statistic 'sum' of propagate_grid\(\) is named twice"),
        (None, None, ["min"], r"The ensemble statistics of propagate_grid\(\) need a list of observables"),
        (obs, ["min"], ["min"], r"The ensemble statistics of propagate_grid\(\) cannot be combined with statistics over the grid"),
        # The checks of the observables keep their messages.
        ([x * v, w + x], None, ALL, "The observable 1 of propagate_grid\\(\\) uses the variable 'w', which is not a state variable"),
        ([hy.par[1] * x], None, ALL, r"An observable of propagate_grid\(\) uses par\[1\], but the integrator has 1 parameter\(s\)"),
        ([], None, ALL, r"The list of observables of propagate_grid\(\) is empty"),
    ]
    for o, st, es, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid([0.0, 1.0], observables=o, statistics=st, ensemble_statistics=es)
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid([0.0, 1.0], observables=o, statistics=st, ensemble_statistics=es, callback=lambda t: True)
        with pytest.raises(ValueError, match=msg):
            ta.propagate_grid_device([0.0, 1.0], 8, observables=o, statistics=st, ensemble_statistics=es)
        with pytest.raises(ValueError, match=msg):
            ta.grid_observables_module(o, statistics=st, ensemble_statistics=es)
        if "parameter" not in msg:  # (without an integrator there is no parameter array to check against)
            with pytest.raises(ValueError, match=msg):
                hy.grid_observables_source(sys_, o, statistics=st, ensemble_statistics=es)
    assert np.all(ta.time == 0.0)
    src, co = ta.grid_observables_module(obs, ensemble_statistics=ALL)
    assert "hy_ens_merge" in src and co[:4] == b"\x7fELF"
    # One module per list, and per way of merging.
    assert ta.grid_observables_module(obs, ensemble_statistics=list(ALL)) == (src, co)
    assert ta.grid_observables_module(obs, ensemble_statistics=["count"])[0] != src
    assert ta.grid_observables_module(obs)[0] != src and "hy_ens" not in ta.grid_observables_module(obs)[0]


def test_c_abi():
    lib = _lib.lib
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -x)]
    s = hy._to_sys(sys_)
    obs = [x * v]
    arr = (ctypes.c_void_p * 1)(obs[0]._h)
    null = (ctypes.c_void_p * 1)(None)
    codes = (ctypes.c_int * 6)(*range(6))
    err = lambda: lib.hy_last_error().decode()  # noqa: E731
    p = lib.hy_grid_ens_source(s._h, arr, 1, codes, 6, 20, 1)
    assert p and _lib.take_str(p) == hy.grid_observables_source(sys_, obs, order=20, high_accuracy=True, ensemble_statistics=ALL)
    assert not lib.hy_grid_ens_source(None, arr, 1, codes, 6, 20, 0) and err() == "hy_grid_ens_source(): the system handle is null"
    assert not lib.hy_grid_ens_source(s._h, null, 1, codes, 6, 20, 0)
    assert err() == "hy_grid_ens_source(): the observable 0 is a null expression"
    assert not lib.hy_grid_ens_source(s._h, arr, 1, None, 6, 20, 0) and err() == "hy_grid_ens_source(): the array of statistics is null"
    assert not lib.hy_grid_ens_source(s._h, arr, 1, (ctypes.c_int * 2)(0, 6), 2, 20, 0)
    assert err() == "The ensemble statistic code 6 of propagate_grid() is unknown"
    assert not lib.hy_grid_ens_source(s._h, arr, 1, (ctypes.c_int * 2)(4, 4), 2, 20, 0)
    assert err() == "The ensemble statistic 'sum_sq' of propagate_grid() is named twice"
    assert not lib.hy_grid_ens_source(s._h, arr, 1, codes, 0, 20, 0)
    assert err() == "The list of ensemble statistics of propagate_grid() is empty"
    ta = hy.taylor_adaptive_batch(sys_, None, 4)
    grid = (ctypes.c_double * 8)(*([0.0] * 4 + [1.0] * 4))
    assert lib.hy_grid_ens_acc_words(2, 1, codes, 6) == 2 * 139
    assert lib.hy_grid_ens_acc_words(2, 1, (ctypes.c_int * 1)(9), 1) == 0
    assert err() == "The ensemble statistic code 9 of propagate_grid() is unknown"
    acc = (ctypes.c_uint64 * (2 * 139))()
    invalid = lib.hy_tab_propagate_grid_ens(None, grid, 2, 0, None, 0, None, 0, arr, 1, codes, 6, acc)
    assert invalid != 0 and err() == "hy_tab_propagate_grid_ens(): the integrator handle is null"
    assert lib.hy_tab_propagate_grid_ens(ta._h, grid, 2, 0, None, 0, None, 0, arr, 1, None, 6, acc) == invalid
    assert err() == "hy_tab_propagate_grid_ens(): the array of statistics is null"
    assert lib.hy_tab_propagate_grid_ens_device(ta._h, grid, 2, 0, 0, None, 0, arr, 1, codes, 6, None) == invalid
    assert err() == "hy_tab_propagate_grid_ens_device(): the device output pointer is null"
    assert lib.hy_tab_grid_ens_module(None, arr, 1, codes, 6, None, None, None) == invalid
    assert err() == "hy_tab_grid_ens_module(): the integrator handle is null"
    assert lib.hy_tab_grid_ens_module(ta._h, arr, 1, codes, 6, None, None, None) == 0
    assert lib.hy_grid_ens_add(acc, 2, 1, codes, 6, 2, 0, 1.0) == invalid
    assert err() == "hy_grid_ens_add(): the record (2, 0) is outside the accumulators"
    # init, add, merge, finish on the host.
    other = (ctypes.c_uint64 * (2 * 139))()
    out = (ctypes.c_double * 12)()
    assert lib.hy_grid_ens_init(acc, 2, 1, codes, 6) == 0 and lib.hy_grid_ens_init(other, 2, 1, codes, 6) == 0
    assert lib.hy_grid_ens_add(acc, 2, 1, codes, 6, 1, 0, 1e308) == 0 and lib.hy_grid_ens_add(other, 2, 1, codes, 6, 1, 0, -1e308) == 0
    assert lib.hy_grid_ens_add(other, 2, 1, codes, 6, 1, 0, 0.5) == 0
    assert lib.hy_grid_ens_merge(acc, other, 2, 1, codes, 6) == 0 and lib.hy_grid_ens_finish(acc, 2, 1, codes, 6, out) == 0
    assert same(list(out), ref_stats([], ALL) + ref_stats([1e308, -1e308, 0.5], ALL))
    hdr = open(os.path.join(ROOT, "include", "heyoka_amd.h")).read()
    for k, name in enumerate(ALL):
        assert "#define HY_ENS_STAT_%s %d\n" % (name.upper(), k) in hdr
    assert list(hy.ENSEMBLE_STATISTICS) == ALL


def build_cpp():
    """tests/cpp/test_grid_ensemble.cpp, compiled the way tests/test_grid_statistics.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_grid_ensemble.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_grid_ensemble_host_half():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
