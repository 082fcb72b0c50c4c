// The event log through the C++ interface: the tag type event_recorder in place of a callback of nt_event_batch<double> /
// t_event_batch<double>, get_event_log() / get_event_log_size() / clear_event_log(). Written against the reference's
// include layout and namespace. The host half type-checks the interface and runs everything which needs no device; the
// GPU half compares the log of an integrator with recorders with what callbacks of the caller's see.
// usage: test_event_recorder [gpu]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include <heyoka/events.hpp>
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

void host_half()
{
    static_assert(std::is_constructible_v<nte_t, expression, event_recorder>);
    static_assert(std::is_default_constructible_v<event_recorder>);
    auto [x, v] = make_vars("x", "v");
    nte_t e0(v, event_recorder{});
    nte_t e1(x - 0.01, event_recorder{}, kw::direction = event_direction::positive);
    nte_t plain(v, [](tab &, double, int, std::uint32_t) {});
    te_t t0(x, kw::callback = event_recorder{}, kw::cooldown = 0.05);
    te_t t_plain(x, kw::callback = [](tab &, int, std::uint32_t) { return true; });
    CHECK(e0.is_recorder() && e1.is_recorder() && !plain.is_recorder());
    CHECK(e1.get_direction() == event_direction::positive);
    CHECK(t0.is_recorder() && !t_plain.is_recorder() && t0.get_cooldown() == 0.05);
    CHECK(static_cast<bool>(t0.get_callback()) && static_cast<bool>(e0.get_callback()));

    tab ta({prime(x) = v, prime(v) = -9.8 * sin(x)}, initial_state(), bs, kw::nt_events = {e0, e1}, kw::t_events = {t0});
    CHECK(ta.with_events());
    CHECK(ta.get_event_log_size() == 0u);
    CHECK(ta.get_event_log().empty());
    CHECK(ta.get_event_log_row_size() == 8u + ta.get_dim());
    ta.clear_event_log();
    CHECK(ta.get_event_log_size() == 0u);
    // The copy has an empty log too.
    tab tb(ta);
    CHECK(tb.get_event_log_size() == 0u && tb.get_event_log_row_size() == 10u);
    // An integrator without recorders: a log of size zero.
    tab tc({prime(x) = v, prime(v) = -9.8 * sin(x)}, initial_state(), bs, kw::nt_events = {plain});
    CHECK(tc.get_event_log_size() == 0u && tc.get_event_log().empty());
    std::printf("HOST OK (%d checks)\n", n_checks);
}

void gpu_half()
{
    auto [x, v] = make_vars("x", "v");
    struct seen {
        std::uint32_t lane;
        int cls, idx, d_sgn;
        double t;
    };
    std::vector<seen> log;
    tab a({prime(x) = v, prime(v) = -9.8 * sin(x)}, initial_state(), bs,
          kw::nt_events = {nte_t(v, event_recorder{}), nte_t(x - 0.01, event_recorder{})},
          kw::t_events = {te_t(x, kw::callback = event_recorder{}, kw::cooldown = 0.05)});
    tab b({prime(x) = v, prime(v) = -9.8 * sin(x)}, initial_state(), bs,
          kw::nt_events = {nte_t(v, [&](tab &, double t, int d, std::uint32_t i) { log.push_back({i, 1, 0, d, t}); }),
                           nte_t(x - 0.01, [&](tab &, double t, int d, std::uint32_t i) { log.push_back({i, 1, 1, d, t}); })},
          kw::t_events = {te_t(
                              x,
                              kw::callback =
                                  [&](tab &, int d, std::uint32_t i) {
                                      log.push_back({i, 0, 0, d, std::nan("")});
                                      return true;
                                  },
                              kw::cooldown = 0.05)});
    for (int s = 0; s < 10; ++s) {
        a.step();
        b.step();
        CHECK(a.get_state() == b.get_state());
        CHECK(a.get_time() == b.get_time());
    }
    const auto w = a.get_event_log_row_size();
    CHECK(w == 10u);
    const auto rows = a.get_event_log();
    CHECK(a.get_event_log_size() == log.size());
    CHECK(rows.size() == log.size() * w);
    CHECK(log.size() > 8u);
    int n_term = 0;
    for (std::size_t r = 0; r < log.size(); ++r) {
        const auto *row = rows.data() + r * w;
        CHECK(row[0] == log[r].lane && row[1] == log[r].cls && row[2] == log[r].idx && row[3] == log[r].d_sgn);
        if (log[r].cls == 1) {
            CHECK(row[4] == log[r].t);
        } else {
            ++n_term;
            // (The terminal event x = 0: the state at the event.)
            CHECK(std::abs(row[8]) < 1e-14);
        }
        CHECK(std::isfinite(row[8]) && std::isfinite(row[9]) && row[7] >= 0.);
    }
    CHECK(n_term > 0);
    a.clear_event_log();
    CHECK(a.get_event_log_size() == 0u && a.get_event_log().empty());
    a.step();
    std::printf("GPU OK (%d checks, %zu rows)\n", n_checks, log.size());
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
