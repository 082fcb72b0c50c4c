// Grid observables through the <heyoka/...> include layout: kw::observables on propagate_grid() and on
// ensemble_propagate_grid_batch(). Host side (no GPU): the checks against the system, which come before any device use, and
// the module of the observables. With the argument "gpu": the observables of a grid against cfunc<double> of the same
// expressions over the full output of the same call without observables, bit for bit, and the size of the result.
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

static constexpr unsigned N = 3, DIM = 2;

static taylor_adaptive_batch<double> make(double shift = 0.)
{
    auto [x, v] = make_vars("x", "v");
    return taylor_adaptive_batch<double>{{prime(x) = v, prime(v) = -par[0] * x},
                                         {1. + shift, 1.5, 2., 0., 0.1, 0.2},
                                         N,
                                         kw::pars = std::vector<double>{1., 1.5, 2.5}};
}

static std::vector<expression> observables()
{
    auto [x, v] = make_vars("x", "v");
    return {0.5 * (v * v + par[0] * x * x) + 1e-3 * sin(heyoka::time), x * v};
}

static void host_checks()
{
    auto [x, v, w] = make_vars("x", "v", "w");
    auto ta = make();
    const std::vector<double> grid{0., 0., 0., 1., 1., 1.};
    // Before any device use: the integrator has not created its device objects when these throw.
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = std::vector<expression>{}),
                 "The list of observables of propagate_grid() is empty");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = std::vector<expression>{x * v, w * x}),
                 "The observable 1 of propagate_grid() uses the variable 'w', which is not a state variable of the system");
    CHECK_THROWS(ta.propagate_grid(grid, kw::observables = {par[2] * x}),
                 "An observable of propagate_grid() uses par[2], but the integrator has 1 parameter(s)");
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t) { return t; };
    CHECK_THROWS(ensemble_propagate_grid_batch(ta, std::vector<double>{0., 1.}, 2, gen, kw::observables = {w}),
                 "The observable 0 of propagate_grid() uses the variable 'w', which is not a state variable of the system");
    // The module: two columns, both rows, the three kernels; the same text for a copy.
    const auto obs = observables();
    const detail::grid_sampling gs(obs);
    const auto &src = ta.core().grid_sampling_module(gs).source;
    CHECK(src.find("#define HY_NOUT 2u") != std::string::npos);
    CHECK(src.find("hy_grid_post(") != std::string::npos && src.find("hy_grid_obs0(") != std::string::npos
          && src.find("hy_grid_unsample(") != std::string::npos);
    CHECK(!ta.core().grid_sampling_module(gs).code.empty());
    auto tb = ta;
    CHECK(tb.core().grid_sampling_module(gs).source == src);
    std::puts("HOST OK");
}

// cfunc(obs) over every row of a full grid output against the observable output of the same grid.
static void check_rows(const std::vector<double> &full, const std::vector<double> &out, const std::vector<double> &grid,
                       const std::vector<double> &pars)
{
    auto [x, v] = make_vars("x", "v");
    const auto obs = observables();
    const auto n_grid = grid.size() / N;
    CHECK(full.size() == n_grid * DIM * N);
    CHECK(out.size() == n_grid * obs.size() * N);
    cfunc<double> cf(obs, {x, v});
    for (std::size_t g = 0; g < n_grid; ++g) {
        const std::vector<double> in(full.begin() + g * DIM * N, full.begin() + (g + 1u) * DIM * N);
        const std::vector<double> tm(grid.begin() + g * N, grid.begin() + (g + 1u) * N);
        std::vector<double> ref(obs.size() * N);
        cf(ref, in, kw::pars = pars, kw::time = tm);
        for (const auto r : ref) {
            CHECK(std::isfinite(r));
        }
        CHECK(std::memcmp(ref.data(), out.data() + g * obs.size() * N, ref.size() * sizeof(double)) == 0);
    }
}

static void gpu_checks()
{
    const auto obs = observables();
    const std::vector<double> pars{1., 1.5, 2.5};
    // Per-lane grids, grid[point * N + lane].
    std::vector<double> grid;
    for (unsigned p = 0; p < 5u; ++p) {
        for (unsigned i = 0; i < N; ++i) {
            grid.push_back(p * (1. + 0.1 * i));
        }
    }
    auto ta = make(), tb = make();
    auto [cb_a, full] = ta.propagate_grid(grid);
    auto [cb_b, out] = tb.propagate_grid(grid, kw::observables = obs);
    CHECK(!cb_a && !cb_b);
    check_rows(full, out, grid, pars);
    CHECK(ta.get_state() == tb.get_state() && ta.get_time() == tb.get_time());
    CHECK(ta.get_propagate_res() == tb.get_propagate_res());
    // A braced list and max_steps: the rows which were not reached are NaN in both columns.
    {
        auto [x, v] = make_vars("x", "v");
        auto tc = make();
        auto [cb_c, o2] = tc.propagate_grid(grid, kw::max_steps = 2, kw::observables = {x * v, v});
        CHECK(o2.size() == 5u * 2u * N);
        CHECK(!std::isnan(o2[0]) && std::isnan(o2[4u * 2u * N]) && std::isnan(o2[4u * 2u * N + N]));
    }
    // The ensemble driver, three iterations with different initial conditions, a scalar grid.
    const std::vector<double> sgrid{0., 0.7, 1.9, 3.};
    std::vector<double> splat;
    for (const auto t : sgrid) {
        splat.insert(splat.end(), N, t);
    }
    const auto gen = [](taylor_adaptive_batch<double> t, std::size_t i) {
        t.get_state_data()[0] += 0.25 * static_cast<double>(i);
        return t;
    };
    const auto base = make();
    auto ret_full = ensemble_propagate_grid_batch(base, sgrid, 3, gen);
    auto ret_obs = ensemble_propagate_grid_batch(base, sgrid, 3, gen, kw::observables = obs);
    CHECK(ret_full.size() == 3u && ret_obs.size() == 3u);
    for (std::size_t i = 0; i < 3u; ++i) {
        check_rows(std::get<2>(ret_full[i]), std::get<2>(ret_obs[i]), splat, pars);
        CHECK(std::get<0>(ret_full[i]).get_state() == std::get<0>(ret_obs[i]).get_state());
    }
    CHECK(std::get<2>(ret_obs[0]) != std::get<2>(ret_obs[1]));
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
