// Terminal-event actions (event_action) through the C++ interface and the C ABI, written against the
// reference's include layout and namespace. The host half checks what needs no device: the tag type as kw::callback of
// t_event_batch<double>, the error messages of the construction, where the events are applied, copies. The GPU half
// bounces a batch of harmonic oscillators at x = 0 (v <- -0.8 v) and compares with the same integrator whose callback is
// a lambda doing the same multiplication on the host.
// usage: test_event_action [gpu]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <utility>
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
using nte_t = nt_event_batch<double>;
using pairs_t = std::vector<std::pair<expression, expression>>;

const std::vector<double> amps = {0.5, 1.1, 0.9};

std::vector<double> initial_state()
{
    const auto n = amps.size();
    std::vector<double> st(2u * n, 0.);
    for (std::size_t i = 0; i < n; ++i) {
        st[i] = amps[i];
    }
    return st;
}

tab with_action(const pairs_t &a, int semantics = 0)
{
    auto [x, v] = make_vars("x", "v");
    return tab({prime(x) = v, prime(v) = -x}, initial_state(), static_cast<std::uint32_t>(amps.size()),
               kw::batch_semantics = semantics,
               kw::t_events = {te_t(x, kw::callback = event_action(a), kw::direction = event_direction::negative)});
}

bool rejected(const pairs_t &a, const std::string &what)
{
    try {
        with_action(a);
    } catch (const std::invalid_argument &e) {
        return std::string(e.what()).find(what) != std::string::npos;
    }
    return false;
}

void host_half()
{
    auto [x, v] = make_vars("x", "v");
    const auto q = make_vars("q");
    for (int s : {0, 3}) {
        auto ta = with_action({{v, -0.8 * v}}, s);
        CHECK(ta.with_events());
        CHECK(ta.events_on_device());
        // A copy keeps the action.
        auto tb = ta;
        CHECK(tb.events_on_device());
    }
    CHECK(rejected({}, "empty list of assignments"));
    CHECK(rejected({{v, 1. * x}, {v, 2. * x}}, "assigned more than once"));
    CHECK(rejected({{q, 1. * x}}, "is not a state variable of the system"));
    CHECK(rejected({{x + v, 1. * x}}, "is not a state variable of the system"));
    CHECK(rejected({{v, q * x}}, "uses the variable 'q', which is not a state variable"));
    CHECK(rejected({{v, par[0] * x}}, "uses par[0]"));
    CHECK(event_action(pairs_t{{v, -0.8 * v}}).to_string().rfind("event_action({v: ", 0) == 0u);
    {
        // Next to a callback of the caller's the integrator keeps the host loop.
        auto ta = tab({prime(x) = v, prime(v) = -x}, initial_state(), static_cast<std::uint32_t>(amps.size()),
                      kw::t_events = {te_t(x, kw::callback = event_action(pairs_t{{v, -0.8 * v}}))},
                      kw::nt_events = {nte_t(v, [](tab &, double, int, std::uint32_t) {})});
        CHECK(!ta.events_on_device());
    }
    // The C ABI: handle, clone, repr, the checks of either stage.
    hy_expr hx = hy_expr_var("x"), hv = hy_expr_var("v"), hnum = hy_expr_num(-0.8);
    hy_expr hr = hy_expr_mul(hnum, hv);
    hy_event_action a = hy_event_action_new(&hv, &hr, 1);
    CHECK(a != nullptr);
    hy_event_action b = hy_event_action_clone(a);
    CHECK(b != nullptr);
    char *sa = hy_event_action_str(a), *sb = hy_event_action_str(b);
    CHECK(std::string(sa) == sb && std::string(sa).rfind("event_action({v: ", 0) == 0u);
    hy_free_str(sa);
    hy_free_str(sb);
    CHECK(hy_event_action_new(&hv, &hr, 0) == nullptr);
    CHECK(std::string(hy_last_error()).find("empty list of assignments") != std::string::npos);
    CHECK(hy_event_action_new(&hr, &hr, 1) == nullptr);
    CHECK(std::string(hy_last_error()).find("is not a variable") != std::string::npos);
    hy_sys sys = hy_model_pendulum(9.8, 1.);
    CHECK(sys != nullptr);
    {
        // (The pendulum's state variables are x and v.)
        hy_t_event te{};
        te.eq = hx;
        te.cb = hy_event_action_t;
        te.user = a;
        te.direction = 0;
        te.cooldown = -1;
        hy_tab t = hy_tab_create_with_events(sys, nullptr, 0, 4, nullptr, &te, 1, nullptr, 0);
        CHECK(t != nullptr);
        // The integrator holds its own copy of the action.
        hy_event_action_free(a);
        CHECK(hy_tab_events_on_device(t) == 1 && hy_tab_n_event_actions(t) == 1u);
        hy_tab t2 = hy_tab_copy(t);
        CHECK(t2 != nullptr && hy_tab_events_on_device(t2) == 1 && hy_tab_n_event_actions(t2) == 1u);
        char *src = nullptr;
        const char *co = nullptr;
        size_t co_size = 0;
        CHECK(hy_tab_event_action_module(t2, &src, &co, &co_size) == 0);
        CHECK(std::string(src).find("hy_ev_action") != std::string::npos && co != nullptr && co_size > 0u);
        hy_free_str(src);
        hy_tab_free(t2);
        hy_tab_free(t);
        // A left-hand side which is no state variable of THIS system.
        hy_expr hq = hy_expr_var("q");
        hy_event_action c = hy_event_action_new(&hq, &hr, 1);
        CHECK(c != nullptr);
        te.user = c;
        CHECK(hy_tab_create_with_events(sys, nullptr, 0, 4, nullptr, &te, 1, nullptr, 0) == nullptr);
        CHECK(std::string(hy_last_error()).find("is not a state variable of the system") != std::string::npos);
        hy_event_action_free(c);
        hy_expr_free(hq);
    }
    hy_event_action_free(b);
    hy_sys_free(sys);
    hy_expr_free(hr);
    hy_expr_free(hnum);
    hy_expr_free(hv);
    hy_expr_free(hx);
    std::printf("HOST OK (%d checks)\n", n_checks);
}

void gpu_half()
{
    auto [x, v] = make_vars("x", "v");
    const auto n = static_cast<std::uint32_t>(amps.size());
    auto ta = with_action({{v, -0.8 * v}});
    auto tl = tab({prime(x) = v, prime(v) = -x}, initial_state(), n,
                  kw::t_events = {te_t(x, kw::callback = [n](tab &t, int, std::uint32_t i) {
                                            t.get_state_data()[n + i] *= -0.8;
                                            return true;
                                        },
                                        kw::direction = event_direction::negative)});
    CHECK(ta.events_on_device() && !tl.events_on_device());
    // x = A cos t goes down through 0 at pi / 2: the bounce is within the first steps.
    unsigned bounces = 0;
    for (int k = 0; k < 12; ++k) {
        ta.step();
        tl.step();
        for (std::uint32_t i = 0; i < n; ++i) {
            CHECK(ta.get_step_res()[i] == tl.get_step_res()[i]);
            bounces += std::get<0>(ta.get_step_res()[i]) == taylor_outcome{0} ? 1u : 0u;
            CHECK(ta.get_time()[i] == tl.get_time()[i]);
        }
        for (std::uint32_t j = 0; j < 2u * n; ++j) {
            CHECK(ta.get_state()[j] == tl.get_state()[j]);
        }
    }
    CHECK(bounces >= n);
    ta.propagate_until(10.);
    tl.propagate_until(10.);
    for (std::uint32_t i = 0; i < n; ++i) {
        CHECK(ta.get_propagate_res()[i] == tl.get_propagate_res()[i]);
        CHECK(std::get<0>(ta.get_propagate_res()[i]) == taylor_outcome::time_limit && ta.get_time()[i] == 10.);
    }
    for (std::uint32_t j = 0; j < 2u * n; ++j) {
        CHECK(ta.get_state()[j] == tl.get_state()[j]);
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
