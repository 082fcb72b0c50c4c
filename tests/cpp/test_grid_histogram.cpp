// Ensemble histograms through the <heyoka/...> include layout: kw::ensemble_histograms next to kw::observables on
// propagate_grid() - alone and with kw::ensemble_statistics - with kw::histogram_raw, and on ensemble_propagate_grid_batch() with
// kw::histogram_result over three iterations. Host side (no GPU): the refusals, which come before any device use, the module
// which counts, and the counters on a case known by hand. With the argument "gpu": the counters of a grid against this
// program's own binning - a linear scan over the edges, which shares nothing with the library's search - of the output of
// the same call with kw::observables alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include <heyoka/heyoka.hpp>

using namespace heyoka;

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond);                                    \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (false)

template <typename F>
static void check_throws(F &&f, const std::string &msg, int line)
{
    try {
        f();
    } catch (const std::invalid_argument &e) {
        if (msg != e.what()) {
            std::fprintf(stderr, "line %d: wrong message: '%s'\n", line, e.what());
            std::exit(1);
        }
        return;
    }
    std::fprintf(stderr, "line %d: no std::invalid_argument was thrown\n", line);
    std::exit(1);
}
#define CHECK_THROWS(expr, msg) check_throws([&]() { (void)(expr); }, msg, __LINE__)

static constexpr unsigned N = 4;
using es = ensemble_statistic;
using edge_lists = std::vector<std::vector<double>>;

static taylor_adaptive_batch<double> make(double shift = 0.)
{
    auto [x, v] = make_vars("x", "v");
    return taylor_adaptive_batch<double>{{prime(x) = v, prime(v) = -par[0] * x},
                                         {1. + shift, 1.5, 2., -0.5, 0., 0.1, 0.2, 0.3},
                                         N,
                                         kw::pars = std::vector<double>{1., 1.5, 2.5, 0.5}};
}

static std::vector<expression> observables()
{
    auto [x, v] = make_vars("x", "v");
    return {0.5 * (v * v + par[0] * x * x) + 1e-3 * sin(heyoka::time), x * v, log(x)};
}

// Histograms for the first and the third observable: 4 + 2 bins, 6 + 4 = 10 words per grid point.
static const edge_lists all_edges{{0., 0.5, 1., 2., 4.}, {}, {-1., 0., 1.}};
static const std::vector<es> some_stats{es::count, es::mean};

// The counters of y[(g * n_obs + o) * N + i] by a linear scan over the edges.
static std::vector<std::uint64_t> scan(const std::vector<std::vector<double>> &ys, std::size_t n_grid, std::size_t n_obs)
{
    std::size_t words = 0;
    for (const auto &e : all_edges) {
        words += e.empty() ? 0u : e.size() + 1u;
    }
    std::vector<std::uint64_t> acc(n_grid * words, 0u);
    for (const auto &y : ys) {
        CHECK(y.size() == n_grid * n_obs * N);
        for (std::size_t g = 0; g < n_grid; ++g) {
            std::size_t off = 0;
            for (std::size_t o = 0; o < n_obs; ++o) {
                const auto &e = all_edges[o];
                if (e.empty()) {
                    continue;
                }
                for (unsigned i = 0; i < N; ++i) {
                    const double v = y[(g * n_obs + o) * N + i];
                    if (v != v) {
                        continue;
                    }
                    std::size_t s = 0;
                    for (const auto edge : e) {
                        s += edge <= v ? 1u : 0u;
                    }
                    acc[g * words + off + s] += 1u;
                }
                off += e.size() + 1u;
            }
        }
    }
    return acc;
}

static void host_checks()
{
    auto [x, v, w] = make_vars("x", "v", "w");
    auto ta = make();
    const auto obs = observables();
    const std::vector<double> grid{0., 0., 0., 0., 1., 1., 1., 1.};
    CHECK_THROWS(ta.propagate_grid(grid, kw::ensemble_histograms = all_edges),
                 "The ensemble histograms of propagate_grid() need a list of observables");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::statistics = {grid_statistic::min},
                                   kw::ensemble_histograms = all_edges),
                 "The ensemble histograms of propagate_grid() cannot be combined with statistics over the grid");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_histograms = edge_lists{{0., 1.}}),
                 "The ensemble histograms of propagate_grid() need one list of bin edges per observable: 3 observable(s), 1 list(s)");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_histograms = edge_lists{{}, {}, {}}),
                 "The ensemble histograms of propagate_grid() have no bin edges for any observable");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_histograms = edge_lists{{}, {2.}, {}}),
                 "The bin edges of observable 1 of propagate_grid() must be at least 2 finite, strictly increasing values");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = some_stats,
                                   kw::ensemble_histograms = edge_lists{{}, {}, {0., 1., 1.}}),
                 "The bin edges of observable 2 of propagate_grid() must be at least 2 finite, strictly increasing values");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_histograms = edge_lists{{0., INFINITY}, {}, {}}),
                 "The bin edges of observable 0 of propagate_grid() must be at least 2 finite, strictly increasing values");
    std::vector<double> many(4098);
    for (std::size_t k = 0; k < many.size(); ++k) {
        many[k] = static_cast<double>(k);
    }
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_histograms = edge_lists{many, {}, {}}),
                 "The bin edges of observable 0 of propagate_grid() make 4097 bins: at most 4096");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = std::vector<expression>{x * v, w * x, x}, kw::ensemble_histograms = all_edges),
                 "The observable 1 of propagate_grid() uses the variable 'w', which is not a state variable of the system");
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t) { return t; };
    std::vector<std::uint64_t> merged;
    CHECK_THROWS(ensemble_propagate_grid_batch(ta, std::vector<double>{0., 1.}, 2, gen, kw::ensemble_histograms = all_edges,
                                               kw::histogram_result = &merged),
                 "The ensemble histograms of propagate_grid() need a list of observables");
    // The module: 10 words per grid point, no hy_grid_unsample, another module than the one of the observables alone, the same
    // module for other edges.
    const detail::grid_sampling gs(obs, {}, {}, all_edges);
    const auto src = ta.core().grid_sampling_module(gs).source;
    CHECK(src.find("#define HY_NOUT 3u") != std::string::npos && src.find("#define HY_HIST_W 10u") != std::string::npos);
    CHECK(src.find("hy_grid_post(") != std::string::npos && src.find("hy_grid_obs0(") != std::string::npos
          && src.find("hy_grid_unsample(") == std::string::npos);
    CHECK(src != ta.core().grid_sampling_module(detail::grid_sampling(obs)).source);
    CHECK(src == ta.core().grid_sampling_module(detail::grid_sampling(obs, {}, {}, edge_lists{{1., 2., 3., 4., 5.}, {}, {7., 8., 9.}})).source);
    CHECK(!ta.core().grid_sampling_module(gs).code.empty());
    const auto both = ta.core().grid_sampling_module(detail::grid_sampling(obs, {}, some_stats, all_edges)).source;
    CHECK(both.find("#define HY_ENS_WORDS 69u") != std::string::npos && both.find("#define HY_HIST_W 10u") != std::string::npos);
    // The counters on the host.
    const auto lay = detail::hist_layout_of(all_edges);
    CHECK(lay.words == 10u && lay.n_edges == 8u && lay.off[2] == 6u && lay.edge_off[2] == 5u && lay.bins[1] == 0u);
    const auto table = detail::hist_edge_table(all_edges);
    auto a = detail::hist_init(lay, 2), b = detail::hist_init(lay, 2);
    for (const double y : {-1., 0., 0.49, 0.5, 3.9, 4., std::nan(""), static_cast<double>(INFINITY), -0.}) {
        detail::hist_add(lay, table.data(), a.data() + lay.words, 0, y);
    }
    detail::hist_add(lay, table.data(), b.data() + lay.words, 0, 1.5);
    detail::hist_add(lay, table.data(), b.data() + lay.words, 1, 1.5);
    detail::hist_add(lay, table.data(), b.data(), 2, -0.5);
    detail::hist_merge(lay, a.data(), b.data(), 2);
    const std::vector<std::uint64_t> expect{0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 3, 1, 1, 1, 2, 0, 0, 0, 0};
    CHECK(a == expect);
    CHECK(detail::hist_rank_slot(lay, a.data() + lay.words, 0, 1) == 0 && detail::hist_rank_slot(lay, a.data() + lay.words, 0, 2) == 1
          && detail::hist_rank_slot(lay, a.data() + lay.words, 0, 9) == 5 && detail::hist_rank_slot(lay, a.data() + lay.words, 0, 10) == -1
          && detail::hist_rank_slot(lay, a.data() + lay.words, 0, 0) == -1 && detail::hist_rank_slot(lay, a.data(), 2, 1) == 1);
    std::puts("HOST OK");
}

static void gpu_checks()
{
    const auto obs = observables();
    std::vector<double> grid;
    for (unsigned p = 0; p < 9u; ++p) {
        for (unsigned i = 0; i < N; ++i) {
            grid.push_back(p * 0.6 * (1. + 0.1 * i));
        }
    }
    auto ta = make(), tb = make(), tc = make();
    auto [cb_a, y] = ta.propagate_grid(grid, kw::observables = obs);
    std::vector<std::uint64_t> raw, raw2, ens_raw;
    auto [cb_b, out] = tb.propagate_grid(grid, kw::observables = obs, kw::ensemble_histograms = all_edges, kw::histogram_raw = &raw);
    CHECK(!cb_a && !cb_b);
    const auto expect = scan({y}, 9, obs.size());
    CHECK(raw == expect && out.size() == raw.size());
    for (std::size_t k = 0; k < raw.size(); ++k) {
        CHECK(out[k] == static_cast<double>(raw[k]));
    }
    CHECK(ta.get_state() == tb.get_state() && ta.get_time() == tb.get_time());
    CHECK(ta.get_propagate_res() == tb.get_propagate_res());
    // With ensemble statistics: their values first, the same counters behind them.
    auto [cb_c, out2] = tc.propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = some_stats,
                                          kw::ensemble_histograms = all_edges, kw::histogram_raw = &raw2, kw::ensemble_raw = &ens_raw);
    auto [cb_d, out3] = make().propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = some_stats);
    CHECK(raw2 == expect && ens_raw.size() == 9u * 3u * 69u && out2.size() == out3.size() + raw2.size());
    for (std::size_t k = 0; k < out3.size(); ++k) {
        CHECK(out2[k] == out3[k] || (std::isnan(out2[k]) && std::isnan(out3[k])));
    }
    for (std::size_t k = 0; k < raw2.size(); ++k) {
        CHECK(out2[out3.size() + k] == static_cast<double>(raw2[k]));
    }
    CHECK(ta.get_state() == tc.get_state() && ta.get_propagate_res() == tc.get_propagate_res());
    // The ensemble driver: every iteration returns its own counters, kw::histogram_result their sum.
    const std::vector<double> sgrid{0., 0.7, 1.9, 3., 3.1};
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t i) {
        t.get_state_data()[0] += 0.25 * static_cast<double>(i);
        return t;
    };
    const auto base = make();
    std::vector<std::uint64_t> merged;
    auto ret_obs = ensemble_propagate_grid_batch(base, sgrid, 3, gen, kw::observables = obs);
    auto ret_h = ensemble_propagate_grid_batch(base, sgrid, 3, gen, kw::observables = obs, kw::ensemble_histograms = all_edges,
                                               kw::histogram_result = &merged);
    CHECK(ret_obs.size() == 3u && ret_h.size() == 3u);
    std::vector<std::vector<double>> ys;
    for (std::size_t i = 0; i < 3u; ++i) {
        const auto one = scan({std::get<2>(ret_obs[i])}, sgrid.size(), obs.size());
        const auto &got = std::get<2>(ret_h[i]);
        CHECK(got.size() == one.size());
        for (std::size_t k = 0; k < one.size(); ++k) {
            CHECK(got[k] == static_cast<double>(one[k]));
        }
        CHECK(std::get<0>(ret_obs[i]).get_state() == std::get<0>(ret_h[i]).get_state());
        ys.push_back(std::get<2>(ret_obs[i]));
    }
    CHECK(merged == scan(ys, sgrid.size(), obs.size()));
    std::uint64_t total = 0;
    for (std::size_t k = 0; k < 6u; ++k) {
        total += merged[k];
    }
    CHECK(total == 12u);
    std::puts("GPU OK");
}

int main(int argc, char **argv)
{
    host_checks();
    if (argc > 1 && std::string(argv[1]) == "gpu") {
        gpu_checks();
    }
    return 0;
}
