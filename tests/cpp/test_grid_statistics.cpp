// Grid statistics through the <heyoka/...> include layout: kw::statistics next to kw::observables on propagate_grid() and on
// ensemble_propagate_grid_batch(). Host side (no GPU): the checks of the list of statistics, which come before any device
// use, and the module which folds. With the argument "gpu": the statistics of a grid against this program's own loop over
// the output of the same call with kw::observables alone, bit for bit, and the size of the result.
#include <cmath>
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
using gs = grid_statistic;

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

static const std::vector<gs> all_stats{gs::min, gs::max, gs::t_min, gs::t_max, gs::sum, gs::last, gs::count};

static void host_checks()
{
    auto [x, v, w] = make_vars("x", "v", "w");
    auto ta = make();
    const auto obs = observables();
    const std::vector<double> grid{0., 0., 0., 0., 1., 1., 1., 1.};
    // Before any device use: the integrator has not created its device objects when these throw.
    CHECK_THROWS(ta.propagate_grid(grid, kw::statistics = all_stats), "The statistics of propagate_grid() need a list of observables");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::statistics = std::vector<gs>{}),
                 "The list of statistics of propagate_grid() is empty");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::statistics = {gs::min, static_cast<gs>(7)}),
                 "The statistic code 7 of propagate_grid() is unknown");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = obs, kw::statistics = {gs::t_max, gs::sum, gs::t_max}),
                 "The statistic 't_max' of propagate_grid() is named twice");
    // (The checks of the observables keep their messages.)
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = std::vector<expression>{x * v, w * x}, kw::statistics = all_stats),
                 "The observable 1 of propagate_grid() uses the variable 'w', which is not a state variable of the system");
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t) { return t; };
    CHECK_THROWS(ensemble_propagate_grid_batch(ta, std::vector<double>{0., 1.}, 2, gen, kw::observables = obs,
                                               kw::statistics = {gs::last, gs::last}),
                 "The statistic 'last' of propagate_grid() is named twice");
    CHECK_THROWS(ensemble_propagate_grid_batch(ta, std::vector<double>{0., 1.}, 2, gen, kw::statistics = all_stats),
                 "The statistics of propagate_grid() need a list of observables");
    // The module: the three kernels, 14 accumulators per lane; t_min alone keeps the minimum in a hidden slot; another module
    // than the one of the observables alone, and the same text for a copy.
    const detail::grid_sampling folded(obs, all_stats);
    const auto &src = ta.core().grid_sampling_module(folded).source;
    CHECK(src.find("#define HY_NOUT 2u") != std::string::npos && src.find("#define HY_NSLOT 14u") != std::string::npos);
    CHECK(src.find("hy_grid_post(") != std::string::npos && src.find("hy_grid_obs0(") != std::string::npos
          && src.find("hy_grid_unsample(") != std::string::npos);
    CHECK(ta.core().grid_sampling_module(detail::grid_sampling(obs, std::vector<gs>{gs::t_min})).source.find("#define HY_NSLOT 4u")
          != std::string::npos);
    CHECK(src != ta.core().grid_sampling_module(detail::grid_sampling(obs)).source);
    CHECK(!ta.core().grid_sampling_module(folded).code.empty());
    auto tb = ta;
    CHECK(tb.core().grid_sampling_module(folded).source == src);
    std::puts("HOST OK");
}

static bool same_bits(double a, double b)
{
    return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(double)) == 0;
}

// The statistics of the output y[(g * n_obs + o) * N + i] of the call with the observables alone - the rows which are not NaN
// in every column, a prefix of the grid - against out[(o * n_stat + k) * N + i].
static void check_fold(const std::vector<double> &y, const std::vector<double> &out, const std::vector<double> &grid,
                       std::size_t n_obs)
{
    const auto n_grid = grid.size() / N;
    const auto n_stat = all_stats.size();
    CHECK(y.size() == n_grid * n_obs * N);
    CHECK(out.size() == n_obs * n_stat * N);
    for (unsigned i = 0; i < N; ++i) {
        std::size_t r = 0;
        for (; r < n_grid; ++r) {
            bool all_nan = true;
            for (std::size_t o = 0; o < n_obs; ++o) {
                all_nan = all_nan && std::isnan(y[(r * n_obs + o) * N + i]);
            }
            if (all_nan) {
                break;
            }
        }
        for (std::size_t o = 0; o < n_obs; ++o) {
            const double nan = std::nan("");
            double st[7] = {nan, nan, nan, nan, nan, nan, 0.};
            for (std::size_t g = 0; g < r; ++g) {
                const double v = y[(g * n_obs + o) * N + i], t = grid[g * N + i];
                if (g == 0u) {
                    st[0] = st[1] = st[4] = st[5] = v;
                    st[2] = st[3] = t;
                    st[6] = 1.;
                    continue;
                }
                if (v < st[0] || st[0] != st[0]) {
                    st[0] = v;
                    st[2] = t;
                }
                if (v > st[1] || st[1] != st[1]) {
                    st[1] = v;
                    st[3] = t;
                }
                volatile double s = st[4] + v;
                st[4] = s;
                st[5] = v;
                st[6] += 1.;
            }
            for (std::size_t k = 0; k < n_stat; ++k) {
                CHECK(same_bits(out[(o * n_stat + k) * N + i], st[static_cast<int>(all_stats[k])]));
            }
        }
    }
}

static void gpu_checks()
{
    const auto obs = observables();
    // Per-lane grids, grid[point * N + lane].
    std::vector<double> grid;
    for (unsigned p = 0; p < 9u; ++p) {
        for (unsigned i = 0; i < N; ++i) {
            grid.push_back(p * 0.6 * (1. + 0.1 * i));
        }
    }
    auto ta = make(), tb = make();
    auto [cb_a, y] = ta.propagate_grid(grid, kw::observables = obs);
    auto [cb_b, out] = tb.propagate_grid(grid, kw::observables = obs, kw::statistics = all_stats);
    CHECK(!cb_a && !cb_b);
    check_fold(y, out, grid, obs.size());
    // (Every point was reached.)
    CHECK(out[6u * N] == 9. && out[(7u + 6u) * N + N - 1u] == 9.);
    CHECK(ta.get_state() == tb.get_state() && ta.get_time() == tb.get_time());
    CHECK(ta.get_propagate_res() == tb.get_propagate_res());
    // max_steps: the statistics of the prefix which was reached.
    {
        auto tc = make(), td = make();
        auto [cb_c, y2] = tc.propagate_grid(grid, kw::max_steps = 3, kw::observables = obs);
        auto [cb_d, o2] = td.propagate_grid(grid, kw::max_steps = 3, kw::observables = obs, kw::statistics = all_stats);
        check_fold(y2, o2, grid, obs.size());
        CHECK(o2[6u * N] >= 1. && o2[6u * N] < 9.);
        CHECK(tc.get_state() == td.get_state() && tc.get_propagate_res() == td.get_propagate_res());
    }
    // The ensemble driver, two iterations of four systems with different initial conditions, a scalar grid.
    const std::vector<double> sgrid{0., 0.7, 1.9, 3., 3.1};
    std::vector<double> splat;
    for (const auto t : sgrid) {
        splat.insert(splat.end(), N, t);
    }
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t i) {
        t.get_state_data()[0] += 0.25 * static_cast<double>(i);
        return t;
    };
    const auto base = make();
    auto ret_obs = ensemble_propagate_grid_batch(base, sgrid, 2, gen, kw::observables = obs);
    auto ret_st = ensemble_propagate_grid_batch(base, sgrid, 2, gen, kw::observables = obs, kw::statistics = all_stats);
    CHECK(ret_obs.size() == 2u && ret_st.size() == 2u);
    for (std::size_t i = 0; i < 2u; ++i) {
        check_fold(std::get<2>(ret_obs[i]), std::get<2>(ret_st[i]), splat, obs.size());
        CHECK(std::get<0>(ret_obs[i]).get_state() == std::get<0>(ret_st[i]).get_state());
    }
    CHECK(std::get<2>(ret_st[0]) != std::get<2>(ret_st[1]));
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
