// Event-log observables through the C++ interface: set_event_log_observables() / get_event_log_observables() /
// clear_event_log_observables() of taylor_adaptive_batch<double>. Written against the reference's include layout and
// namespace. The host half runs everything which needs no device; the GPU half runs an integrator with the state columns
// and one with the observables from the same initial data and holds every observable column to cfunc of the state columns,
// the parameters of the row's system and the trigger time of the row, bit for bit.
// usage: test_event_observables [gpu]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <heyoka/events.hpp>
#include <heyoka/expression.hpp>
#include <heyoka/heyoka.hpp>
#include <heyoka/kw.hpp>
#include <heyoka/taylor.hpp>

using namespace heyoka;

namespace
{

int n_checks = 0;

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        ++n_checks;                                                                                                    \
        if (!(cond)) {                                                                                                 \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);                              \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (0)

using tab = taylor_adaptive_batch<double>;
using te_t = t_event_batch<double>;
using nte_t = nt_event_batch<double>;

constexpr std::uint32_t bs = 8;

std::vector<double> initial_state()
{
    std::vector<double> st(2u * bs);
    for (std::uint32_t i = 0; i < bs; ++i) {
        st[i] = -0.2 + 0.03 * i;
        st[bs + i] = 1.5 + 0.1 * i;
    }
    return st;
}

// (One gravity per system: the parameters matter.)
std::vector<double> parameters()
{
    std::vector<double> p(bs);
    for (std::uint32_t i = 0; i < bs; ++i) {
        p[i] = 9.8 + 0.05 * i;
    }
    return p;
}

tab make(bool recorders = true)
{
    auto [x, v] = make_vars("x", "v");
    if (!recorders) {
        return tab({prime(x) = v, prime(v) = -par[0] * sin(x)}, initial_state(), bs, kw::pars = parameters(),
                   kw::nt_events = {nte_t(v, [](tab &, double, int, std::uint32_t) {})});
    }
    return tab({prime(x) = v, prime(v) = -par[0] * sin(x)}, initial_state(), bs, kw::pars = parameters(),
               kw::nt_events = {nte_t(v, event_recorder{}), nte_t(x - 0.01, event_recorder{})},
               kw::t_events = {te_t(x, kw::callback = event_recorder{}, kw::cooldown = 0.05)});
}

std::vector<expression> observables()
{
    auto [x, v] = make_vars("x", "v");
    return {0.5 * v * v - par[0] * cos(x), sin(x), heyoka::time, v};
}

template <typename F>
std::string message_of(const F &f)
{
    try {
        f();
    } catch (const std::invalid_argument &e) {
        return e.what();
    }
    return {};
}

void host_half()
{
    auto [x, v] = make_vars("x", "v");
    auto ta = make();
    CHECK(ta.get_event_log_observables().empty() && ta.get_event_log_row_size() == 10u);
    ta.set_event_log_observables(observables());
    CHECK(ta.get_event_log_observables() == observables() && ta.get_event_log_row_size() == 12u);
    tab tb(ta);
    CHECK(tb.get_event_log_observables() == observables() && tb.get_event_log_row_size() == 12u);
    ta.clear_event_log_observables();
    CHECK(ta.get_event_log_observables().empty() && ta.get_event_log_row_size() == 10u && tb.get_event_log_row_size() == 12u);
    CHECK(message_of([&] { ta.set_event_log_observables({}); }).find("is empty") != std::string::npos);
    CHECK(message_of([&] { ta.set_event_log_observables({x * make_vars("q")}); }).find("not a state variable") != std::string::npos);
    CHECK(message_of([&] { ta.set_event_log_observables({x * par[1]}); }).find("par[1]") != std::string::npos);
    auto tc = make(false);
    CHECK(message_of([&] { tc.set_event_log_observables({x}); }).find("no recording event callbacks") != std::string::npos);
    std::printf("HOST OK (%d checks)\n", n_checks);
}

void gpu_half()
{
    auto [x, v] = make_vars("x", "v");
    auto s = make(), o = make();
    o.set_event_log_observables(observables());
    for (int k = 0; k < 10; ++k) {
        s.step();
        o.step();
        CHECK(s.get_state() == o.get_state());
        CHECK(s.get_time() == o.get_time());
    }
    const auto ws = s.get_event_log_row_size(), wo = o.get_event_log_row_size();
    CHECK(ws == 10u && wo == 12u);
    const auto n = s.get_event_log_size();
    CHECK(n > 8u && o.get_event_log_size() == n);
    const auto rs = s.get_event_log(), ro = o.get_event_log();
    // cfunc of the state columns: inputs[var * n + row], one parameter and one time per row.
    std::vector<double> in(2u * n), ps(n), tm(n), out(4u * n);
    const auto pars = parameters();
    int n_term = 0, n_nt = 0;
    for (std::uint64_t r = 0; r < n; ++r) {
        CHECK(std::memcmp(rs.data() + r * ws, ro.data() + r * wo, 8u * sizeof(double)) == 0);
        in[r] = rs[r * ws + 8u];
        in[n + r] = rs[r * ws + 9u];
        ps[r] = pars[static_cast<std::size_t>(rs[r * ws])];
        tm[r] = rs[r * ws + 4u];
        (rs[r * ws + 1u] == 0. ? n_term : n_nt) += 1;
    }
    CHECK(n_term > 0 && n_nt > 0);
    cfunc<double> cf(observables(), {x, v});
    cf(out, in, kw::pars = ps, kw::time = tm);
    for (std::uint64_t r = 0; r < n; ++r) {
        for (std::uint32_t k = 0; k < 4u; ++k) {
            CHECK(std::memcmp(&out[k * n + r], &ro[r * wo + 8u + k], sizeof(double)) == 0);
        }
    }
    // The setter is refused on a non-empty log, and accepted once the log is cleared.
    CHECK(message_of([&] { o.clear_event_log_observables(); }).find("only while the log is empty") != std::string::npos);
    o.clear_event_log();
    o.clear_event_log_observables();
    CHECK(o.get_event_log_row_size() == 10u);
    o.step();
    std::printf("GPU OK (%d checks, %llu rows)\n", n_checks, static_cast<unsigned long long>(n));
}

} // namespace

int main(int argc, char **argv)
{
    host_half();
    if (argc > 1 && std::string(argv[1]) == "gpu") {
        gpu_half();
    }
    return 0;
}
