// step_action through the <heyoka/...> include layout: construction, copy, stream text, the type-erased callback slot and
// the error messages (host side, no GPU), and - with the argument "gpu" - the action on the device: alone (path 4), in
// sets, with a stop condition, through the ensemble driver, against the same thing written as a host callback. The
// assignment used for the comparisons, v <- 0.5 v, is exact in every arithmetic: the host callback needs no cfunc.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <heyoka/callback/angle_reducer.hpp>
#include <heyoka/callback/step_action.hpp>
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

using assignments_t = std::vector<std::pair<expression, expression>>;

static void host_checks()
{
    auto [x, v, w] = make_vars("x", "v", "w");
    // The constructor: a left-hand side which is not a variable, nothing at all.
    CHECK_THROWS(step_action(assignments_t{{x + v, v}}),
                 "The left-hand side '" + (x + v).to_string() + "' of an assignment of a step action is not a variable");
    CHECK_THROWS(step_action(assignments_t{}), "Cannot construct a step action with neither assignments nor a stop condition");
    // Text, copy, stream.
    const step_action a(assignments_t{{v, 0.5 * v}}, gt(x, 2_dbl));
    const auto txt = a.to_string();
    CHECK(txt.rfind("step_action({v: ", 0) == 0u && txt.find("stop_when=") != std::string::npos);
    const step_action b(a);
    std::ostringstream oss;
    oss << b;
    CHECK(oss.str() == txt);
    const step_action only_cond(gt(x, 2_dbl));
    CHECK(only_cond.get_assignments().empty() && only_cond.get_stop_when());
    CHECK(only_cond.to_string().rfind("step_action({}, stop_when=", 0) == 0u);
    // The callback slot: recognised by type, alone and in sets.
    step_callback_batch<double> cb(a);
    CHECK(value_isa<step_action>(cb));
    CHECK(detail::callback_is_library_action(cb));
    const auto user = [](taylor_adaptive_batch<double> &) { return true; };
    step_callback_batch<double> s1(step_callback_batch_set<double>{a, callback::angle_reducer({x})});
    step_callback_batch<double> s2(step_callback_batch_set<double>{a, user});
    step_callback_batch<double> s3(step_callback_batch_set<double>{callback::angle_reducer({x})});
    CHECK(detail::callback_is_library_action(s1) && !detail::callback_is_library_action(s2)
          && !detail::callback_is_library_action(s3));
    CHECK(!detail::callback_is_library_action(step_callback_batch<double>(user)));
    // The checks against the system, at the first meeting with an integrator (no GPU is touched before they fail).
    auto ta = taylor_adaptive_batch<double>{{prime(x) = v, prime(v) = -x}, {0.1, 0.2, 0., 0.}, 2u};
    CHECK_THROWS(step_action(assignments_t{{w, v}})(ta),
                 "The left-hand side 'w' of an assignment of a step action is not a state variable of the system");
    CHECK_THROWS(step_action(assignments_t{{v, x}, {v, v}})(ta), "The state variable 'v' is assigned more than once by a step action");
    CHECK_THROWS(step_action(assignments_t{{v, w}})(ta), "The right-hand side of the assignment to 'v' of a step action uses the "
                                                         "variable 'w', which is not a state variable of the system");
    CHECK_THROWS(step_action(gt(w, 1_dbl))(ta),
                 "The stop condition of a step action uses the variable 'w', which is not a state variable of the system");
    CHECK_THROWS(step_action(assignments_t{{v, par[1] * v}})(ta), "A step action uses par[1], but the integrator has 0 parameter(s)");
    CHECK_THROWS(ta.propagate_until(1., kw::callback = step_action(assignments_t{{w, v}})),
                 "The left-hand side 'w' of an assignment of a step action is not a state variable of the system");
    // ... at any depth of nested sets.
    step_callback_batch_set<double> inner{step_action(assignments_t{{w, v}}), user};
    CHECK_THROWS(ta.propagate_until(1., kw::callback = step_callback_batch_set<double>{user, inner}),
                 "The left-hand side 'w' of an assignment of a step action is not a state variable of the system");
    std::puts("HOST OK");
}

static void gpu_checks()
{
    auto [x, v] = make_vars("x", "v");
    const auto make = [&](int semantics = 0) {
        return taylor_adaptive_batch<double>{{prime(x) = v, prime(v) = -x}, {1., 1.5, 2., 0., 0., 0.}, 3u, kw::batch_semantics = semantics};
    };
    // (Final times spread: the first system is done several sweeps before the last one - the action must leave it alone.)
    const std::vector<double> tf{1., 4., 9.};
    const auto host_half = [](taylor_adaptive_batch<double> &t) {
        const auto lh = t.get_last_h();
        auto *st = t.get_state_data();
        for (unsigned i = 0; i < 3u; ++i) {
            if (lh[i] != 0) {
                st[3u + i] *= 0.5;
            }
        }
        return true;
    };
    const step_action half(assignments_t{{v, 0.5 * v}});
    // Direct call on a fresh integrator: nothing happens.
    {
        auto t0 = make();
        const auto st = t0.get_state();
        CHECK(step_action(half)(t0));
        CHECK(t0.get_state() == st);
    }
    auto ta = make(), tb = make();
    auto [c_out, cb] = ta.propagate_until(tf, kw::callback = half);
    CHECK(!c_out && value_isa<step_action>(cb));
    CHECK(ta.core().get_last_callback_path() == 4);
    tb.propagate_until(tf, kw::callback = host_half);
    CHECK(tb.core().get_last_callback_path() == 1);
    CHECK(ta.get_state() == tb.get_state());
    CHECK(ta.get_time() == tb.get_time());
    CHECK(ta.get_propagate_res() == tb.get_propagate_res());
    // Sets: a user callback after the action sees the changed state; the path is 1, the numbers are the same.
    {
        auto tc = make();
        int n_calls = 0;
        tc.propagate_until(tf, kw::callback = step_callback_batch_set<double>{half, [&n_calls](taylor_adaptive_batch<double> &) {
                                                                                  ++n_calls;
                                                                                  return true;
                                                                              }});
        CHECK(n_calls > 3 && tc.core().get_last_callback_path() == 1);
        CHECK(tc.get_state() == tb.get_state());
        auto td = make();
        td.propagate_grid({0., 0., 0., 1., 4., 9.}, kw::callback = half);
        CHECK(td.core().get_last_callback_path() == 4);
        CHECK(td.get_state() == tb.get_state());
    }
    // Stop condition, default semantics: the loop ends like after a host callback which returned false.
    {
        const step_action stop(gt(-x, 0.5_dbl));
        auto te = make(), tf2 = make();
        te.propagate_until(20., kw::callback = stop);
        tf2.propagate_until(20., kw::callback = [](taylor_adaptive_batch<double> &t) {
            const auto &st = t.get_state();
            bool go = true;
            for (unsigned i = 0; i < 3u; ++i) {
                go = go && !(-st[i] > 0.5);
            }
            return go;
        });
        CHECK(te.get_state() == tf2.get_state() && te.get_time() == tf2.get_time());
        CHECK(te.get_propagate_res() == tf2.get_propagate_res());
        for (const auto &r : te.get_propagate_res()) {
            CHECK(std::get<0>(r) == taylor_outcome::cb_stop);
        }
        CHECK(te.core().get_n_stopped_by_action() == 0u);
    }
    // Independent semantics: the systems with x^2 + v^2 > 1.5 (amplitudes 1.5 and 2) stop alone after their first step, the
    // first one (amplitude 1) runs to its end.
    {
        auto tg = make(3);
        tg.propagate_until(20., kw::callback = step_action(gt(x * x + v * v, 1.5_dbl)));
        const auto &res = tg.get_propagate_res();
        CHECK(std::get<0>(res[0]) == taylor_outcome::time_limit);
        CHECK(std::get<0>(res[1]) == taylor_outcome::cb_stop && std::get<0>(res[2]) == taylor_outcome::cb_stop);
        CHECK(tg.core().get_n_stopped_by_action() == 2u && tg.get_n_retired() == 0u);
        CHECK(tg.get_time()[0] == 20. && tg.get_time()[1] < 20. && tg.get_time()[2] < 20.);
    }
    // The ensemble driver copies the (stateless) action into every iteration.
    {
        const auto base = make();
        const auto gen = [](taylor_adaptive_batch<double> t, std::size_t) { return t; };
        auto ret = ensemble_propagate_until_batch(base, 4., 2, gen, kw::callback = half);
        auto th = make();
        th.propagate_until(4., kw::callback = half);
        CHECK(ret.size() == 2u);
        for (auto &r : ret) {
            CHECK(std::get<0>(r).get_state() == th.get_state());
            CHECK(value_isa<step_action>(std::get<2>(r)));
        }
    }
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
