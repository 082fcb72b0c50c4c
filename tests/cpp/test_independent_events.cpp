// The independent semantics (kw::batch_semantics = 3, hy_tab_config::batch_semantics = 3) through the C++ interface and
// the C ABI: within one propagate_until() a stopping terminal event retires ONE system, the others carry on. Written
// against the reference's include layout and namespace. The host half checks what needs no device (the value is accepted
// at both boundaries, 4 and 7 are rejected, where the events are applied); the GPU half runs a batch of harmonic
// oscillators with the terminal event x = 1 (no callback) against the same systems run alone under the default semantics.
// usage: test_independent_events [gpu]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include <heyoka/events.hpp>
#include <heyoka/heyoka.hpp>
#include <heyoka/kw.hpp>
#include <heyoka/taylor.hpp>

#include <heyoka_amd.h>

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

// Amplitudes below and above 1: x(t) = A cos t goes down through 1 at acos(1 / A) if A > 1, never otherwise.
const std::vector<double> amps = {0.5, 1.1, 0.9, 1.5, 3.0};

tab make(const std::vector<double> &a, int semantics)
{
    auto [x, v] = make_vars("x", "v");
    const auto n = static_cast<std::uint32_t>(a.size());
    std::vector<double> st(2u * n, 0.);
    for (std::uint32_t i = 0; i < n; ++i) {
        st[i] = a[i];
    }
    return tab({prime(x) = v, prime(v) = -x}, st, n, kw::batch_semantics = semantics,
               kw::t_events = {te_t(x - 1., kw::direction = event_direction::negative)});
}

bool rejected(int semantics)
{
    try {
        make(amps, semantics);
    } catch (const std::invalid_argument &e) {
        return std::string(e.what()).rfind("Invalid batch semantics", 0) == 0u
               && std::string(e.what()).find("3 independent") != std::string::npos;
    }
    return false;
}

void host_half()
{
    // kw::batch_semantics: 0 .. 3 accepted; a plain stop is applied on the device under the new value only.
    for (int s = 0; s <= 3; ++s) {
        auto ta = make(amps, s);
        CHECK(ta.with_events());
        CHECK(ta.events_on_device() == (s == 3));
        CHECK(ta.get_n_retired() == 0u);
    }
    CHECK(rejected(4));
    CHECK(rejected(7));
    CHECK(rejected(-1));
    // hy_tab_config of the C ABI.
    hy_sys sys = hy_model_pendulum(9.8, 1.);
    CHECK(sys != nullptr);
    for (int s : {3, 4, 7}) {
        hy_tab_config cfg{};
        cfg.batch_semantics = s;
        hy_tab t = hy_tab_create(sys, nullptr, 0, 4, &cfg);
        if (s == 3) {
            CHECK(t != nullptr);
            CHECK(hy_tab_get_n_retired(t) == 0u);
            CHECK(hy_tab_events_on_device(t) == 0);
            hy_tab_free(t);
        } else {
            CHECK(t == nullptr);
            CHECK(std::string(hy_last_error()).rfind("Invalid batch semantics", 0) == 0u);
        }
    }
    hy_sys_free(sys);
    std::printf("HOST OK (%d checks)\n", n_checks);
}

void gpu_half()
{
    auto ta = make(amps, 3);
    ta.propagate_until(10.);
    const auto &res = ta.get_propagate_res();
    std::uint64_t n_ret = 0;
    for (std::size_t i = 0; i < amps.size(); ++i) {
        // The system alone, default semantics.
        auto solo = make({amps[i]}, 0);
        solo.propagate_until(10.);
        const auto &sres = solo.get_propagate_res();
        CHECK(res[i] == sres[0]);
        CHECK(ta.get_state()[i] == solo.get_state()[0]);
        CHECK(ta.get_state()[amps.size() + i] == solo.get_state()[1]);
        CHECK(ta.get_time()[i] == solo.get_time()[0]);
        const auto oc = std::get<0>(res[i]);
        if (amps[i] > 1.) {
            ++n_ret;
            CHECK(static_cast<std::int64_t>(oc) == -1);
            // (Closed form; the bound of tests/test_independent_events.py.)
            CHECK(std::abs(ta.get_time()[i] - std::acos(1. / amps[i])) <= 10 * 1.1102230246251565e-16);
            CHECK(std::abs(ta.get_state()[i] - 1.) <= 1e-14);
        } else {
            CHECK(oc == taylor_outcome::time_limit);
            CHECK(ta.get_time()[i] == 10.);
            CHECK(std::get<3>(res[i]) >= 4u);
        }
    }
    CHECK(n_ret == 3u && ta.get_n_retired() == n_ret);
    // The next call starts every system again (the retired ones well before their next crossing at acos(1 / A) + 2 pi).
    const std::vector<double> tf2 = {10.5, 2., 10.5, 2., 2.};
    ta.propagate_until(tf2);
    CHECK(ta.get_n_retired() == 0u);
    for (std::size_t i = 0; i < amps.size(); ++i) {
        CHECK(std::get<0>(ta.get_propagate_res()[i]) == taylor_outcome::time_limit && ta.get_time()[i] == tf2[i]);
    }
    std::printf("GPU OK (%d checks)\n", n_checks);
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
