"""Ensemble histograms: propagate_grid() counts its observables into bins across the systems per grid point.
Host half: the counters - host add, merge, rank_slot, quantile_bracket - against numpy.searchsorted(..., side="right") with a
NaN filter and against a sort of the values; the generated module which counts (hiprtc cross-compiles without a GPU) and its
resources; the refusals in every front end; the C++ program. The numbers of the kernels are checked in
tests/test_grid_histogram_gpu.py, which uses ref_counts() from here."""
import ctypes
import hashlib
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import heyoka_amd as hy
from heyoka_amd import _lib, codegen_check

from test_grid_observables import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "heyoka_amd", "csrc", "_build", "test_grid_histogram")
INF, NAN = float("inf"), float("nan")
TINY = 5e-324
MODES = ["peratomic", "aggregate", "hybrid"]


# ---- the reference: the definition, with numpy ----
def ref_slots(edges, values):
    """(slots of the values which are not NaN)."""
    v = np.asarray(values, dtype=float).reshape(-1)
    return np.searchsorted(np.asarray(edges, dtype=float), v[~np.isnan(v)], side="right")


def ref_record(edges, values):
    """The B + 2 counters of a list of values."""
    return np.bincount(ref_slots(edges, values), minlength=len(edges) + 1).astype(np.uint64)


def ref_counts(edges, y):
    """The counters of y[point, lane], (n_grid, B + 2)."""
    return np.stack([ref_record(edges, row) for row in y])


def around(edges):
    """Every edge and its two neighbours among the doubles."""
    e = np.asarray(edges, dtype=float)
    return np.concatenate([e, np.nextafter(e, -INF), np.nextafter(e, INF)])


EDGES = {
    "one_bin": np.array([-1.0, 2.5]),
    "bins_4096": np.linspace(-3.0, 5.0, 4097),
    "wide": np.array([-1e300, -1e150, -1.0, -1e-300, 0.0, 1e-300, 3.0, 1e10, 1e300]),
    "one_ulp": np.nextafter(1.0, INF) + np.arange(6) * 2.0**-52,
    "zero_edge": np.array([-2.0, 0.0, 2.0]),
    "subnormal": np.array([-TINY, 0.0, TINY, 3 * TINY, 2.0**-1022]),
}
SPECIAL = np.array([0.0, -0.0, INF, -INF, NAN, TINY, -TINY, 2 * TINY, 2.0**-1023, -(2.0**-1040), NAN, 1.0, -1.0, 1e308, -1e308])


def value_list(edges):
    rng = np.random.RandomState(len(edges))
    lo, hi = edges[0], edges[-1]
    with np.errstate(over="ignore"):
        inside = lo / 2 + hi / 2 + (hi / 2 - lo / 2) * rng.uniform(-1.2, 1.2, 300)
    return np.concatenate([around(edges), SPECIAL, inside])


def host_hist(edges, values, n_acc=1):
    """The values dealt over n_acc accumulators, which are merged into the first."""
    accs = [hy.ensemble_histogram_accumulators(1, [edges]) for _ in range(n_acc)]
    for k, v in enumerate(values):
        accs[k % n_acc].add(0, 0, v)
    for a in accs[1:]:
        accs[0].merge(a)
    return accs[0]


@pytest.mark.parametrize("name", sorted(EDGES))
def test_host_twin_is_searchsorted_right_for_any_dealing(name):
    edges = EDGES[name]
    assert np.all(np.diff(edges) > 0)
    vals = value_list(edges)
    exp = ref_record(edges, vals)
    assert exp.sum() == (~np.isnan(vals)).sum() and exp.size == len(edges) + 1
    words = [host_hist(edges, vals, k).raw for k in (1, 2, 7)]
    for w in words:
        assert w.dtype == np.uint64 and np.array_equal(w, exp), name
    # The empty list: counters in their start state.
    assert not host_hist(edges, []).raw.any()


def test_zero_infinities_nan_and_the_open_sides():
    h = hy.ensemble_histogram_accumulators(1, [EDGES["zero_edge"]])
    for v in (-0.0, 0.0):
        h.add(0, 0, v)
    assert list(h.counts(0)[0]) == [0, 0, 2, 0]  # (both zeros in [0, 2))
    h.add(0, 0, -INF).add(0, 0, INF).add(0, 0, NAN).add(0, 0, 2.0).add(0, 0, -2.0).add(0, 0, np.nextafter(-2.0, -INF))
    assert list(h.counts(0)[0]) == [2, 1, 2, 2]


def test_record_sizes_offsets_and_acc_words():
    e = [np.linspace(0, 1, 9), None, np.array([0.0, 1.0]), []]
    h = hy.ensemble_histogram_accumulators(3, e)
    assert h.words == 10 + 3 and h.raw.size == 3 * 13 and h.raw.dtype == np.uint64 and not h.raw.any()
    assert h.counts(0).shape == (3, 10) and h.counts(2).shape == (3, 3)
    assert [x.size for x in h.edges] == [9, 0, 2, 0]
    h.add(2, 2, 0.5).add(1, 0, 5.0).add(1, 1, 0.5).add(0, 3, 0.5)  # (observables without edges are skipped)
    exp = np.zeros((3, 13), dtype=np.uint64)
    exp[2, 11], exp[1, 9] = 1, 1
    assert np.array_equal(h.raw.reshape(3, 13), exp)
    for o in (1, 3, 4):
        with pytest.raises(ValueError, match="has no histogram"):
            h.counts(o)
    narr = (ctypes.c_size_t * 4)(9, 0, 2, 0)
    assert _lib.lib.hy_grid_hist_acc_words(3, 4, narr) == 39
    assert _lib.lib.hy_grid_hist_acc_words(1, 1, (ctypes.c_size_t * 1)(4097)) == 4098
    other = hy.ensemble_histogram_accumulators(3, [np.linspace(0, 2, 9), None, np.array([0.0, 1.0]), None])
    with pytest.raises(ValueError, match="different bin edges"):
        h.merge(other)
    with pytest.raises(ValueError, match="different shapes"):
        h.merge(hy.ensemble_histogram_accumulators(2, e))


def sorted_rank_slot(edges, values, k):
    v = np.sort(np.asarray([x for x in values if x == x], dtype=float))
    if k == 0 or k > v.size:
        return -1
    return int(np.searchsorted(edges, v[k - 1], side="right"))


def test_rank_slot_and_quantile_bracket_against_a_sort():
    edges = np.array([-1.0, 0.0, 0.5, 4.0])
    rng = np.random.RandomState(2)
    lists = [
        list(rng.uniform(-3.0, 6.0, 101)) + [NAN, NAN],
        [-5.0] * 9 + [0.25],  # (most ranks in the underflow slot)
        [7.0] * 9 + [0.25],  # (most ranks in the overflow slot)
        [0.25],
        [],
    ]
    h = hy.ensemble_histogram_accumulators(len(lists), [None, edges])
    for g, vals in enumerate(lists):
        for v in vals:
            h.add(g, 1, v)
    ns = [sum(1 for v in vals if v == v) for vals in lists]
    assert list(h.counts(1).sum(axis=1)) == ns
    for k in (0, 1, 2, 9, 10, 50, 101, 102):
        assert list(h.rank_slot(1, k)) == [sorted_rank_slot(edges, vals, k) for vals in lists], k
    ext = np.concatenate([[-INF], edges, [INF]])
    for q in (0, 1, 0.5, Fraction(1, 3), 0.9, Fraction(9, 10), 0.05, 0.99):
        br = h.quantile_bracket(1, q)
        assert br.shape == (len(lists), 2)
        for g, vals in enumerate(lists):
            if ns[g] == 0:
                assert np.isnan(br[g]).all()
                continue
            k = max(1, math.ceil(Fraction(q) * ns[g]))
            s = sorted_rank_slot(edges, vals, k)
            assert (br[g, 0], br[g, 1]) == (ext[s], ext[s + 1]), (q, g)
            v = sorted(x for x in vals if x == x)[k - 1]
            assert br[g, 0] <= v < br[g, 1] or (v == INF and br[g, 1] == INF)
    # The open sides.
    assert tuple(h.quantile_bracket(1, 0)[1]) == (-INF, -1.0) and tuple(h.quantile_bracket(1, 1)[2]) == (4.0, INF)
    assert tuple(h.quantile_bracket(1, 1)[1]) == (0.0, 0.5) and tuple(h.quantile_bracket(1, 0)[2]) == (0.0, 0.5)
    # A rank per grid point.
    assert list(h.rank_slot(1, [1, 10, 10, 1, 1])) == [sorted_rank_slot(edges, v, k) for v, k in zip(lists, [1, 10, 10, 1, 1])]
    with pytest.raises(ValueError, match="outside"):
        h.quantile_bracket(1, 1.5)


# ---- the generated module ----
def kernel(src, name):
    return src.split("%s(const hy_grid_args a)" % name)[1].split('extern "C"')[0]


HEADLINE = ["count", "mean", "min", "max", "sum_sq"]


def case_edges(obs, shift=0.0):
    return [np.linspace(-1.0, 1.0, 257) + shift] + [None] * (len(obs) - 1)


def check_text(src, plain, merge, ens):
    for k in ("hy_grid_post", "hy_grid_obs0", "hy_until_post", "hy_indep_override"):
        assert 'extern "C" __global__ void __launch_bounds__(256) %s(' % k in src
    assert "hy_grid_unsample" not in src and "__shared__" not in src
    assert "#define HY_HIST_W 258u" in src and "#define HY_HIST_MODE %d\n" % MODES.index(merge) in src
    assert ("#define HY_HIST_ENSW (HY_NOUT * HY_ENS_WORDS)" in src) == ens and ("#define HY_HIST_ENSW 0u" in src) != ens
    assert ("#define HY_ENS_WORDS 139u" in src) == ens
    post, obs0 = kernel(src, "hy_grid_post"), kernel(src, "hy_grid_obs0")
    sec = src.split("void hy_obs_section(")[1].split('extern "C"')[0]
    rows = lambda s: s.split("const double *tcb = tc0;")[1].split("hy_obs_section(a, i, N")[0]  # noqa: E731
    assert rows(post) == rows(kernel(plain, "hy_grid_post"))
    assert 'asm volatile("" : "+v"(y0));' in sec
    assert ("hy_ens_merge((u64 *)outp + ((u64)g * HY_NOUT + 0u) * HY_ENS_WORDS, y0);" in sec) == ens
    assert ("hy_hist_count(hy_hist_rec(outp, a.n_grid, g) + (0u + hy_hist_slot(hy_hist_edges(outp, a.n_grid) + 0u, 257u, 256u, y0)), "
            "y0 == y0);") in sec
    assert "hy_obs_section(a, i, N, a.out, g, tg.hi" in post and "hy_obs_section(a, i, N, a.out, 0u, a.grid[i]" in obs0
    # Integer atomics only, no cross-lane operation but ballots and lane reads.
    assert "atomicAdd(" in src and "unsafeAtomicAdd" not in src and "atomicAdd((double" not in src and "atomicAdd((float" not in src
    hist = src.split("// Ensemble histograms (DESIGN 4.3h)")[1].split("void hy_obs_section(")[0]
    for word in ("dpp", "permute", "shfl", "ds_swizzle"):
        assert word not in hist.lower()


@pytest.mark.parametrize("ens", [False, True])
@pytest.mark.parametrize("merge", MODES)
@pytest.mark.parametrize("mode", ["registers", "staged"])
@pytest.mark.parametrize("ha", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_source_counts_and_compiles_without_scratch(case, ha, mode, merge, ens, monkeypatch):
    monkeypatch.setenv("HEYOKA_AMD_GRID_OBS", mode)
    monkeypatch.setenv("HEYOKA_AMD_GRID_HIST", merge)
    monkeypatch.delenv("HEYOKA_AMD_GRID_HIST_TURNS", raising=False)
    monkeypatch.delenv("HEYOKA_AMD_GRID_ENS", raising=False)
    sys_, obs, n_rows, dim = case()
    kw = dict(ensemble_statistics=HEADLINE) if ens else {}
    src = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha, ensemble_histograms=case_edges(obs), **kw)
    plain = hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha)
    check_text(src, plain, merge, ens)
    # The text does not depend on the values of the edges.
    assert src == hy.grid_observables_source(sys_, obs, order=20, high_accuracy=ha, ensemble_histograms=case_edges(obs, 3.5), **kw)
    co = hy.hiprtc_compile(src)
    assert co[:4] == b"\x7fELF"
    for k in ("hy_grid_post", "hy_grid_obs0"):
        res = codegen_check.kernel_resources(co, kernel=k)
        assert res is not None
        print(case.__name__, ha, mode, merge, ens, k, res, "text sha256 %s" % hashlib.sha256(src.encode()).hexdigest()[:12])
        assert res["scratch_bytes_per_lane"] == 0 and res["vgpr_spill"] == 0 and res["lds_bytes"] == 0, (k, res)
        # (SGPRs parked in lanes of a VGPR - sgpr_spill of the metadata, no memory involved - are printed with the sha256 of
        # the text, not bounded: the same text compiles to different numbers of them depending on what the process compiled
        # before - the staged Horner pair distance: 2 alone, 22 late in a run of the whole suite, the same sha256 -, so a bound
        # on the figure would test the state of the compiler, not this text. DESIGN 4.3h has both sets of figures. What a spill
        # would cost is memory traffic, and that is what is asserted above: no scratch and no VGPR spill.)


def test_the_existing_variants_do_not_change_and_the_switch_is_checked(monkeypatch):
    sys_, obs, _, _ = CASES[0]()
    variants = lambda: (hy.grid_observables_source(sys_, obs), hy.grid_observables_source(sys_, obs, statistics=["min", "sum"]),  # noqa: E731
                        hy.grid_observables_source(sys_, obs, ensemble_statistics=HEADLINE))
    monkeypatch.delenv("HEYOKA_AMD_GRID_HIST", raising=False)
    monkeypatch.delenv("HEYOKA_AMD_GRID_HIST_TURNS", raising=False)
    a = variants()
    default = hy.grid_observables_source(sys_, obs, ensemble_histograms=case_edges(obs))
    monkeypatch.setenv("HEYOKA_AMD_GRID_HIST", "peratomic")
    assert variants() == a and all("hy_hist" not in s and "HY_HIST" not in s for s in a)
    # A module requested without the argument is the text it was: None is no argument.
    assert hy.grid_observables_source(sys_, obs, ensemble_histograms=None) == a[0]
    assert hy.grid_observables_source(sys_, obs, ensemble_statistics=HEADLINE, ensemble_histograms=None) == a[2]
    # The text of the ensemble statistics stands unchanged inside the combined module.
    both = hy.grid_observables_source(sys_, obs, ensemble_statistics=HEADLINE, ensemble_histograms=case_edges(obs))
    ens_text = a[2].split("// Ensemble statistics (DESIGN 4.3g)")[1].split("// The observables of lane i")[0]
    assert ens_text in both
    monkeypatch.setenv("HEYOKA_AMD_GRID_HIST", "hybrid")
    assert hy.grid_observables_source(sys_, obs, ensemble_histograms=case_edges(obs)) == default  # (the default mode)
    # The number of turns of the hybrid mode is a constant of the library, one of the three which were measured;
    # HEYOKA_AMD_GRID_HIST_TURNS, the switch of that measurement, overrides it, is part of the text and is checked.
    built_in = int(default.split("#define HY_HIST_TURNS ")[1].split("u")[0])
    assert built_in in (1, 2, 4)
    for k in (1, 2, 4):
        monkeypatch.setenv("HEYOKA_AMD_GRID_HIST_TURNS", str(k))
        src_k = hy.grid_observables_source(sys_, obs, ensemble_histograms=case_edges(obs))
        assert "#define HY_HIST_TURNS %du\n" % k in src_k and (src_k == default) == (k == built_in)
        assert hy.hiprtc_compile(src_k)[:4] == b"\x7fELF" and variants() == a
    for bad_k in ("3", "0", "two"):
        monkeypatch.setenv("HEYOKA_AMD_GRID_HIST_TURNS", bad_k)
        with pytest.raises(ValueError, match="Invalid value '%s' of HEYOKA_AMD_GRID_HIST_TURNS: '1', '2' or '4'" % bad_k):
            hy.grid_observables_source(sys_, obs, ensemble_histograms=case_edges(obs))
    monkeypatch.setenv("HEYOKA_AMD_GRID_HIST_TURNS", "")
    assert hy.grid_observables_source(sys_, obs, ensemble_histograms=case_edges(obs)) == default
    monkeypatch.setenv("HEYOKA_AMD_GRID_HIST", "sometimes")
    with pytest.raises(ValueError, match="Invalid value 'sometimes' of HEYOKA_AMD_GRID_HIST: 'peratomic', 'aggregate' or 'hybrid'"):
        hy.grid_observables_source(sys_, obs, ensemble_histograms=case_edges(obs))
    assert variants() == a


def test_bin_counts_and_offsets_are_constants_of_the_module():
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -x)]
    obs = [hy.par[0], x * v, v]
    e = [np.array([0.0, 1.0]), None, np.linspace(0.0, 1.0, 4097)]
    src = hy.grid_observables_source(sys_, obs, ensemble_histograms=e)
    assert "#define HY_HIST_W 4101u" in src
    assert "(0u + hy_hist_slot(hy_hist_edges(outp, a.n_grid) + 0u, 2u, 2u, y0))" in src
    assert "(3u + hy_hist_slot(hy_hist_edges(outp, a.n_grid) + 2u, 4097u, 4096u, y2))" in src
    assert "y1 == y1" not in src and src.count("hy_hist_count(hy_hist_rec(") == 2
    assert hy.hiprtc_compile(src)[:4] == b"\x7fELF"
    # Observables of the parameters alone.
    src = hy.grid_observables_source(sys_, [hy.par[0]], ensemble_histograms=[[0.0, 1.0, 2.0]])
    assert "#define HY_NROWS 0u" in src and hy.hiprtc_compile(src)[:4] == b"\x7fELF"


def test_refusals_in_every_front_end():
    x, v, w = hy.make_vars("x", "v", "w")
    sys_ = [(x, v), (v, -hy.par[0] * x)]
    ta = hy.taylor_adaptive_batch(sys_, None, 4)
    obs = [x * v, x]
    ok = [[0.0, 1.0], None]
    two = r"The bin edges of observable %d of propagate_grid\(\) must be at least 2 finite, strictly increasing values"
    bad = [
        (None, None, ok, r"The ensemble histograms of propagate_grid\(\) need a list of observables"),
        (obs, ["min"], ok, r"The ensemble histograms of propagate_grid\(\) cannot be combined with statistics over the grid"),
        (obs, None, [[0.0, 1.0]],
         r"The ensemble histograms of propagate_grid\(\) need one list of bin edges per observable: 2 observable\(s\), 1 list\(s\)"),
        (obs, None, [None, []], r"The ensemble histograms of propagate_grid\(\) have no bin edges for any observable"),
        (obs, None, [None, [1.0]], two % 1),
        (obs, None, [[0.0, 1.0, 1.0], None], two % 0),
        (obs, None, [[0.0, 2.0, 1.0], None], two % 0),
        (obs, None, [None, [0.0, INF]], two % 1),
        (obs, None, [None, [NAN, 1.0]], two % 1),
        (obs, None, [None, np.arange(4098.0)], r"The bin edges of observable 1 of propagate_grid\(\) make 4097 bins: at most 4096"),
        # The checks of the observables keep their messages.
        ([x * v, w + x], None, ok, "The observable 1 of propagate_grid\\(\\) uses the variable 'w', which is not a state variable"),
        ([hy.par[1] * x, x], None, ok, r"An observable of propagate_grid\(\) uses par\[1\], but the integrator has 1 parameter\(s\)"),
    ]
    for o, st, eh, msg in bad:
        for es in (None, ["count"]) if st is None else (None,):
            kw = dict(observables=o, statistics=st, ensemble_statistics=es, ensemble_histograms=eh)
            with pytest.raises(ValueError, match=msg):
                ta.propagate_grid([0.0, 1.0], **kw)
            with pytest.raises(ValueError, match=msg):
                ta.propagate_grid([0.0, 1.0], callback=lambda t: True, **kw)
            with pytest.raises(ValueError, match=msg):
                ta.propagate_grid_device([0.0, 1.0], 8, **kw)
            with pytest.raises(ValueError, match=msg):
                ta.grid_observables_module(o, statistics=st, ensemble_statistics=es, ensemble_histograms=eh)
            if "parameter" not in msg:
                with pytest.raises(ValueError, match=msg):
                    hy.grid_observables_source(sys_, o, statistics=st, ensemble_statistics=es, ensemble_histograms=eh)
    with pytest.raises(ValueError, match=two % 0):
        hy.ensemble_histogram_accumulators(2, [[3.0]])
    assert np.all(ta.time == 0.0)
    src, co = ta.grid_observables_module(obs, ensemble_histograms=ok)
    assert "hy_hist_count" in src and co[:4] == b"\x7fELF"
    # One module per list of bin counts and per way of merging, not per list of edges.
    assert ta.grid_observables_module(obs, ensemble_histograms=[[5.0, 7.0], []]) == (src, co)
    assert ta.grid_observables_module(obs, ensemble_histograms=[[0.0, 1.0, 2.0], None])[0] != src
    assert ta.grid_observables_module(obs, ensemble_histograms=ok, ensemble_statistics=["count"])[0] != src
    assert ta.grid_observables_module(obs)[0] != src and "hy_hist" not in ta.grid_observables_module(obs)[0]
    assert ta.grid_observables_module(obs)[0] == hy.grid_observables_source(sys_, obs)


def test_c_abi():
    lib = _lib.lib
    x, v = hy.make_vars("x", "v")
    sys_ = [(x, v), (v, -x)]
    s = hy._to_sys(sys_)
    obs = [x * v, x]
    arr = (ctypes.c_void_p * 2)(obs[0]._h, obs[1]._h)
    codes = (ctypes.c_int * 2)(0, 5)
    edges = (ctypes.c_double * 5)(0.0, 0.5, 1.0, -1.0, 1.0)
    n_edges = (ctypes.c_size_t * 2)(3, 2)
    e_py = [[0.0, 0.5, 1.0], [-1.0, 1.0]]
    err = lambda: lib.hy_last_error().decode()  # noqa: E731
    for n_stats, es in ((0, None), (2, ["count", "mean"])):
        p = lib.hy_grid_hist_source(s._h, arr, 2, codes, n_stats, edges, n_edges, 20, 1)
        assert p and _lib.take_str(p) == hy.grid_observables_source(sys_, obs, order=20, high_accuracy=True, ensemble_statistics=es,
                                                                    ensemble_histograms=e_py)
    assert not lib.hy_grid_hist_source(None, arr, 2, codes, 0, edges, n_edges, 20, 0)
    assert err() == "hy_grid_hist_source(): the system handle is null"
    assert not lib.hy_grid_hist_source(s._h, arr, 2, codes, 0, edges, None, 20, 0)
    assert err() == "hy_grid_hist_source(): the array of the numbers of bin edges is null"
    assert not lib.hy_grid_hist_source(s._h, arr, 2, codes, 0, None, n_edges, 20, 0)
    assert err() == "hy_grid_hist_source(): the array of bin edges is null"
    assert not lib.hy_grid_hist_source(s._h, arr, 2, None, 2, edges, n_edges, 20, 0)
    assert err() == "hy_grid_hist_source(): the array of statistics is null"
    assert not lib.hy_grid_hist_source(s._h, arr, 2, (ctypes.c_int * 2)(0, 6), 2, edges, n_edges, 20, 0)
    assert err() == "The ensemble statistic code 6 of propagate_grid() is unknown"
    refusals = [
        ((ctypes.c_size_t * 2)(0, 0), edges, "The ensemble histograms of propagate_grid() have no bin edges for any observable"),
        ((ctypes.c_size_t * 2)(3, 1), edges,
         "The bin edges of observable 1 of propagate_grid() must be at least 2 finite, strictly increasing values"),
        ((ctypes.c_size_t * 2)(2, 3), (ctypes.c_double * 5)(0.0, 0.5, 1.0, 1.0, 2.0),
         "The bin edges of observable 1 of propagate_grid() must be at least 2 finite, strictly increasing values"),
        ((ctypes.c_size_t * 2)(2, 2), (ctypes.c_double * 4)(0.0, INF, 0.0, 1.0),
         "The bin edges of observable 0 of propagate_grid() must be at least 2 finite, strictly increasing values"),
        ((ctypes.c_size_t * 2)(0, 4098), (ctypes.c_double * 4098)(*range(4098)),
         "The bin edges of observable 1 of propagate_grid() make 4097 bins: at most 4096"),
    ]
    ta = hy.taylor_adaptive_batch(sys_, None, 4)
    grid = (ctypes.c_double * 8)(*([0.0] * 4 + [1.0] * 4))
    acc = (ctypes.c_uint64 * 16)()
    ens = (ctypes.c_uint64 * 512)()
    invalid = lib.hy_tab_propagate_grid_hist(None, grid, 2, 0, None, 0, None, 0, arr, 2, codes, 0, edges, n_edges, None, acc)
    assert invalid != 0 and err() == "hy_tab_propagate_grid_hist(): the integrator handle is null"
    for ne, ed, msg in refusals:
        assert not lib.hy_grid_hist_source(s._h, arr, 2, codes, 0, ed, ne, 20, 0) and err() == msg
        assert lib.hy_tab_propagate_grid_hist(ta._h, grid, 2, 0, None, 0, None, 0, arr, 2, codes, 0, ed, ne, None, acc) == invalid
        assert err() == msg
        assert lib.hy_tab_propagate_grid_hist_device(ta._h, grid, 2, 0, 0, None, 0, arr, 2, codes, 2, ed, ne, acc) == invalid
        assert err() == msg
        assert lib.hy_tab_grid_hist_module(ta._h, arr, 2, codes, 0, ed, ne, None, None, None) == invalid and err() == msg
        if list(ne) in ([0, 0], [3, 1], [0, 4098]):  # (what the numbers of edges alone show)
            assert lib.hy_grid_hist_acc_words(2, 2, ne) == 0 and err() == msg
    assert lib.hy_tab_propagate_grid_hist(ta._h, grid, 2, 0, None, 0, None, 0, arr, 2, codes, 0, edges, n_edges, None, None) == invalid
    assert err() == "hy_tab_propagate_grid_hist(): the array of the histogram counters is null"
    assert lib.hy_tab_propagate_grid_hist(ta._h, grid, 2, 0, None, 0, None, 0, arr, 2, codes, 0, edges, n_edges, ens, acc) == invalid
    assert "must be null without ensemble statistics" in err()
    assert lib.hy_tab_propagate_grid_hist(ta._h, grid, 2, 0, None, 0, None, 0, arr, 2, codes, 2, edges, n_edges, None, acc) == invalid
    assert "must be null without ensemble statistics" in err()
    assert lib.hy_tab_propagate_grid_hist_device(ta._h, grid, 2, 0, 0, None, 0, arr, 2, codes, 0, edges, n_edges, None) == invalid
    assert err() == "hy_tab_propagate_grid_hist_device(): the device output pointer is null"
    assert lib.hy_tab_grid_hist_module(None, arr, 2, codes, 0, edges, n_edges, None, None, None) == invalid
    assert err() == "hy_tab_grid_hist_module(): the integrator handle is null"
    assert lib.hy_tab_grid_hist_module(ta._h, arr, 2, codes, 0, edges, n_edges, None, None, None) == 0
    assert np.all(ta.time == 0.0)
    # init, add, merge, rank_slot on the host: records of 4 + 3 words per grid point.
    assert lib.hy_grid_hist_acc_words(2, 2, n_edges) == 14
    other = (ctypes.c_uint64 * 16)()
    assert lib.hy_grid_hist_init(acc, 2, 2, n_edges) == 0 and lib.hy_grid_hist_init(other, 2, 2, n_edges) == 0
    assert lib.hy_grid_hist_add(acc, 2, 2, edges, n_edges, 2, 0, 1.0) == invalid
    assert err() == "hy_grid_hist_add(): the record (2, 0) is outside the accumulators"
    for a, g, o, y in ((acc, 1, 0, 0.5), (acc, 1, 0, 0.75), (other, 1, 0, -3.0), (other, 1, 1, 0.0), (other, 0, 1, NAN), (acc, 0, 1, 5.0)):
        assert lib.hy_grid_hist_add(a, 2, 2, edges, n_edges, g, o, y) == 0
    assert lib.hy_grid_hist_merge(acc, other, 2, 2, n_edges) == 0
    assert list(acc)[:14] == [0, 0, 0, 0, 0, 0, 1] + [1, 0, 2, 0, 0, 1, 0]
    slots = (ctypes.c_int64 * 2)()
    assert lib.hy_grid_hist_rank_slot(acc, 2, 2, n_edges, 0, (ctypes.c_uint64 * 2)(1, 2), slots) == 0 and list(slots) == [-1, 2]
    assert lib.hy_grid_hist_rank_slot(acc, 2, 2, n_edges, 1, (ctypes.c_uint64 * 2)(1, 2), slots) == 0 and list(slots) == [2, -1]
    assert lib.hy_grid_hist_rank_slot(acc, 2, 2, n_edges, 2, (ctypes.c_uint64 * 2)(1, 2), slots) == invalid
    hdr = open(os.path.join(ROOT, "include", "heyoka_amd.h")).read()
    for name in ("hy_tab_propagate_grid_hist", "hy_tab_propagate_grid_hist_device", "hy_grid_hist_acc_words", "hy_grid_hist_init",
                 "hy_grid_hist_add", "hy_grid_hist_merge", "hy_grid_hist_rank_slot", "hy_grid_hist_source", "hy_tab_grid_hist_module"):
        assert name + "(" in hdr and hasattr(lib, name)


def build_cpp():
    """tests/cpp/test_grid_histogram.cpp, compiled the way tests/test_grid_ensemble.py compiles its program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_grid_histogram.cpp")
    lib = os.path.join(ROOT, "heyoka_amd", "libheyoka_amd.so")
    if os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(src), os.path.getmtime(lib)):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(
        ["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", EXE,
         "-L" + os.path.join(ROOT, "heyoka_amd"), "-lheyoka_amd", "-Wl,-rpath," + os.path.join(ROOT, "heyoka_amd"),
         "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_cpp_grid_histogram_host_half():
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "HOST OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
