// Ensemble statistics through the <heyoka/...> include layout: kw::ensemble_statistics next to kw::observables on
// propagate_grid() and on ensemble_propagate_grid_batch() with kw::ensemble_result. Host side (no GPU): the refusals, which come
// before any device use, the module which merges, and the accumulators on a case known by hand. With the argument "gpu": the
// values of a grid against this program's own fold - the host twin of the kernel, value by value - of the output of the same
// call with kw::observables alone, bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    return {0.5 * (v * v + par[0] * x * x) + 1e-3 * sin(heyoka::time), x * v};
}

static const std::vector<es> all_stats{es::mean, es::count, es::min, es::max, es::sum, es::sum_sq};

static bool same_bits(double a, double b)
{
    return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(double)) == 0;
}

static void host_checks()
{
    auto [x, v, w] = make_vars("x", "v", "w");
    auto ta = make();
    const auto obs = observables();
    const std::vector<double> grid{0., 0., 0., 0., 1., 1., 1., 1.};
    CHECK_THROWS(ta.propagate_grid(grid, kw::ensemble_statistics = all_stats),
                 "The ensemble statistics of propagate_grid() need a list of observables");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = std::vector<es>{}),
                 "The list of ensemble statistics of propagate_grid() is empty");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = {es::min, static_cast<es>(6)}),
                 "The ensemble statistic code 6 of propagate_grid() is unknown");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = {es::mean, es::sum, es::mean}),
                 "The ensemble statistic 'mean' of propagate_grid() is named twice");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::statistics = {grid_statistic::min},
                                   kw::ensemble_statistics = all_stats),
                 "The ensemble statistics of propagate_grid() cannot be combined with statistics over the grid");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = std::vector<expression>{x * v, w * x}, kw::ensemble_statistics = all_stats),
                 "The observable 1 of propagate_grid() uses the variable 'w', which is not a state variable of the system");
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t) { return t; };
    std::vector<double> merged;
    CHECK_THROWS(ensemble_propagate_grid_batch(ta, std::vector<double>{0., 1.}, 2, gen, kw::observables = obs,
                                               kw::ensemble_statistics = {es::max, es::max}, kw::ensemble_result = &merged),
                 "The ensemble statistic 'max' of propagate_grid() is named twice");
    CHECK_THROWS(ensemble_propagate_grid_batch(ta, std::vector<double>{0., 1.}, 2, gen, kw::ensemble_statistics = all_stats),
                 "The ensemble statistics of propagate_grid() need a list of observables");
    // The module: records of 3 + 2 * 68 words, no hy_grid_unsample, another module than the one of the observables alone.
    const detail::grid_sampling merged_gs(obs, {}, all_stats);
    const auto &src = ta.core().grid_sampling_module(merged_gs).source;
    CHECK(src.find("#define HY_NOUT 2u") != std::string::npos && src.find("#define HY_ENS_WORDS 139u") != std::string::npos);
    CHECK(src.find("hy_grid_post(") != std::string::npos && src.find("hy_grid_obs0(") != std::string::npos
          && src.find("hy_grid_unsample(") == std::string::npos);
    CHECK(src != ta.core().grid_sampling_module(detail::grid_sampling(obs)).source);
    CHECK(!ta.core().grid_sampling_module(merged_gs).code.empty());
    // The accumulators on the host: 1e308 + 1 - 1e308 is 1, and the merge is an integer addition.
    const auto lay = detail::ens_layout_of(all_stats);
    CHECK(lay.words == 139u);
    auto a = detail::ens_init(lay, 1), b = detail::ens_init(lay, 1);
    detail::ens_add(lay, a.data(), 1e308);
    detail::ens_add(lay, a.data(), std::nan(""));
    detail::ens_add(lay, b.data(), 1.);
    detail::ens_add(lay, b.data(), -1e308);
    detail::ens_merge(lay, a.data(), b.data(), 1);
    double out[6];
    detail::ens_finish(lay, all_stats, a.data(), 1, out);
    CHECK(out[0] == 1. / 3. && out[1] == 3. && out[2] == -1e308 && out[3] == 1e308 && out[4] == 1. && std::isinf(out[5]));
    std::puts("HOST OK");
}

// The fold of y[(g * n_obs + o) * n + i] over i with the host twin of the kernel.
static std::vector<double> host_fold(const std::vector<std::vector<double>> &ys, std::size_t n_grid, std::size_t n_obs)
{
    const auto lay = detail::ens_layout_of(all_stats);
    auto acc = detail::ens_init(lay, n_grid * n_obs);
    for (const auto &y : ys) {
        CHECK(y.size() == n_grid * n_obs * N);
        for (std::size_t r = 0; r < n_grid * n_obs; ++r) {
            for (unsigned i = 0; i < N; ++i) {
                detail::ens_add(lay, acc.data() + r * lay.words, y[r * N + i]);
            }
        }
    }
    std::vector<double> out(n_grid * n_obs * all_stats.size());
    detail::ens_finish(lay, all_stats, acc.data(), n_grid * n_obs, out.data());
    return out;
}

static void check_same(const std::vector<double> &a, const std::vector<double> &b)
{
    CHECK(a.size() == b.size());
    for (std::size_t k = 0; k < a.size(); ++k) {
        CHECK(same_bits(a[k], b[k]));
    }
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
    auto ta = make(), tb = make();
    auto [cb_a, y] = ta.propagate_grid(grid, kw::observables = obs);
    std::vector<std::uint64_t> raw;
    auto [cb_b, out] = tb.propagate_grid(grid, kw::observables = obs, kw::ensemble_statistics = all_stats, kw::ensemble_raw = &raw);
    CHECK(!cb_a && !cb_b);
    CHECK(out.size() == 9u * 2u * all_stats.size() && raw.size() == 9u * 2u * 139u);
    check_same(out, host_fold({y}, 9, obs.size()));
    // (Every point was reached by every system: out[(g * n_obs + o) * n_stat + k].)
    CHECK(out[1] == 4. && out[(8u * 2u + 1u) * all_stats.size() + 1u] == 4.);
    CHECK(ta.get_state() == tb.get_state() && ta.get_time() == tb.get_time());
    CHECK(ta.get_propagate_res() == tb.get_propagate_res());
    // max_steps: the count falls along the grid.
    {
        auto tc = make(), td = make();
        auto [cb_c, y2] = tc.propagate_grid(grid, kw::max_steps = 3, kw::observables = obs);
        auto [cb_d, o2] = td.propagate_grid(grid, kw::max_steps = 3, kw::observables = obs, kw::ensemble_statistics = all_stats);
        check_same(o2, host_fold({y2}, 9, obs.size()));
        CHECK(o2[1] == 4. && o2[(8u * 2u) * all_stats.size() + 1u] == 0.);
        CHECK(tc.get_state() == td.get_state() && tc.get_propagate_res() == td.get_propagate_res());
    }
    // The ensemble driver: every iteration returns its own values, kw::ensemble_result the merged ones.
    const std::vector<double> sgrid{0., 0.7, 1.9, 3., 3.1};
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t i) {
        t.get_state_data()[0] += 0.25 * static_cast<double>(i);
        return t;
    };
    const auto base = make();
    std::vector<double> merged;
    auto ret_obs = ensemble_propagate_grid_batch(base, sgrid, 3, gen, kw::observables = obs);
    auto ret_es = ensemble_propagate_grid_batch(base, sgrid, 3, gen, kw::observables = obs, kw::ensemble_statistics = all_stats,
                                                kw::ensemble_result = &merged);
    CHECK(ret_obs.size() == 3u && ret_es.size() == 3u);
    std::vector<std::vector<double>> ys;
    for (std::size_t i = 0; i < 3u; ++i) {
        check_same(std::get<2>(ret_es[i]), host_fold({std::get<2>(ret_obs[i])}, sgrid.size(), obs.size()));
        CHECK(std::get<0>(ret_obs[i]).get_state() == std::get<0>(ret_es[i]).get_state());
        ys.push_back(std::get<2>(ret_obs[i]));
    }
    check_same(merged, host_fold(ys, sgrid.size(), obs.size()));
    CHECK(merged[1] == 12.);
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
