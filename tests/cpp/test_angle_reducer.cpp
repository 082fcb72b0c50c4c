// callback::angle_reducer through the reference's include layout: construction, copy / move, stream text and the error
// messages (host side, no GPU), and - with the argument "gpu" - the cases of the reference's batch test
// (test/angle_reducer.cpp, "batch") on the device: the reducer alone (fused into the propagate kernel), in a set next to a
// user callback, the returned callback and the failure modes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <heyoka/callback/angle_reducer.hpp>
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

static const char *const invalid_msg = "Cannot use an angle_reducer which was default-constructed or moved-from";

static void host_checks()
{
    const auto text = [](const callback::angle_reducer &r) {
        std::ostringstream oss;
        oss << r;
        return oss.str();
    };
    // An empty object stays empty through every kind of copy and move.
    {
        callback::angle_reducer empty;
        CHECK(!empty.is_valid());
        callback::angle_reducer copied(empty), target({expression{"q"}});
        target = empty;
        CHECK(!copied.is_valid() && !target.is_valid());
        callback::angle_reducer moved(std::move(copied));
        target = std::move(moved);
        CHECK(!target.is_valid());
    }
    // Built from names in a container, from expressions in a container, from a braced list: the same object each time.
    {
        const std::vector<std::string> names{"psi", "phi"};
        const std::vector<expression> exprs{expression{"phi"}, expression{"psi"}};
        const callback::angle_reducer from_names(names), from_exprs(exprs);
        const callback::angle_reducer from_list = {"phi", "psi", "phi"};
        CHECK(text(from_names) == "Angle reducer: {phi, psi}");
        CHECK(text(from_exprs) == text(from_names) && text(from_list) == text(from_names));
    }
    // A copy is independent of its source; a move leaves the source unusable and carries the indices along.
    {
        auto [x0, v0] = make_vars("x0", "v0");
        auto ta = taylor_adaptive_batch<double>{{prime(x0) = v0, prime(v0) = -sin(x0)}, std::vector<double>(4, 0.), 2u};
        callback::angle_reducer src({v0});
        src.pre_hook(ta);
        callback::angle_reducer dup(src);
        callback::angle_reducer other({x0});
        other.pre_hook(ta);
        src = other;
        CHECK((dup.get_indices() == std::vector<std::size_t>{1}) && (src.get_indices() == std::vector<std::size_t>{0}));
        src = src;
        CHECK(src.is_valid() && text(src) == "Angle reducer: {x0}");
        callback::angle_reducer taken(std::move(dup));
        CHECK(!dup.is_valid() && (taken.get_indices() == std::vector<std::size_t>{1}));
        other = std::move(taken);
        CHECK(!taken.is_valid() && text(other) == "Angle reducer: {v0}");
    }
    CHECK_THROWS(callback::angle_reducer(std::vector<std::string>{}),
                 "The list of expressions passed to the constructor of angle_reducer cannot be empty");
    CHECK_THROWS(callback::angle_reducer(std::vector{expression{1.}}),
                 "The list of expressions passed to the constructor of angle_reducer can contain only variables");
    CHECK_THROWS(callback::angle_reducer(std::vector{1.f}),
                 "The list of expressions passed to the constructor of angle_reducer can contain only variables");
    auto [x, y] = make_vars("x", "y");
    CHECK_THROWS(callback::angle_reducer({x, x + y}),
                 "The list of expressions passed to the constructor of angle_reducer can contain only variables");
    // Stream text.
    {
        std::ostringstream oss;
        oss << callback::angle_reducer{};
        CHECK(oss.str() == "Angle reducer (default constructed)");
    }
    {
        std::ostringstream oss;
        oss << callback::angle_reducer{{expression{"z"}, expression{"x"}, expression{"y"}, expression{"x"}}};
        CHECK(oss.str() == "Angle reducer: {x, y, z}");
    }
    // A step callback like any other: it fits the type-erased holder and is found again by type.
    {
        step_callback_batch<double> cb(callback::angle_reducer({x}));
        CHECK(cb);
        CHECK(value_isa<callback::angle_reducer>(cb));
        auto cb2 = cb;
        CHECK(value_isa<callback::angle_reducer>(cb2));
    }
    // pre_hook() on the host: the sorted indices of the variables in the system; a default-constructed object refuses.
    {
        auto [x0, v0, x1, v1] = make_vars("x0", "v0", "x1", "v1");
        auto ta = taylor_adaptive_batch<double>{{prime(x0) = v0, prime(x1) = v1, prime(v0) = -sin(x0), prime(v1) = -sin(x1)},
                                                std::vector<double>(8, 0.), 2u};
        callback::angle_reducer ar({x1, x0, expression{"not_there"}});
        ar.pre_hook(ta);
        CHECK((ar.get_indices() == std::vector<std::size_t>{0, 1}));
        callback::angle_reducer ar2({v1});
        ar2.pre_hook(ta);
        CHECK((ar2.get_indices() == std::vector<std::size_t>{3}));
        callback::angle_reducer def;
        CHECK_THROWS(def.pre_hook(ta), invalid_msg);
        CHECK_THROWS(def(ta), invalid_msg);
        // Indices which do not fit the integrator passed to the call operator.
        auto ta1 = taylor_adaptive_batch<double>{{prime(x0) = x0}, {0.05, 0.06}, 2u};
        CHECK_THROWS(ar2(ta1), "Inconsistent state detected in angle_reducer: the last index in the indices vector has a value "
                               "of 3, but the number of state variables is only 1");
    }
    std::puts("angle_reducer host checks OK");
}

static void gpu_checks()
{
    using std::cos;
    const auto eps = std::numeric_limits<double>::epsilon();
    auto [x0, v0, x1, v1] = make_vars("x0", "v0", "x1", "v1");
    const auto make = [&]() {
        return taylor_adaptive_batch<double>{{prime(x0) = v0, prime(x1) = v1, prime(v0) = -sin(x0), prime(v1) = -sin(x1)},
                                             {0.05, 0.06, 0.05, 0.05, 10., 10.01, 10.1, 10.11},
                                             2u};
    };
    const auto energy = [](const std::vector<double> &s, int lane, int pend) {
        return 0.5 * s[(2 + pend) * 2 + lane] * s[(2 + pend) * 2 + lane] + (1 - cos(s[pend * 2 + lane]));
    };
    // The reference's batch test: the reducer in a set next to a user callback (host callback loop, reduction on the device).
    auto ta = make();
    const auto st0 = ta.get_state();
    int n_calls = 0;
    step_callback_batch_set<double> scs{callback::angle_reducer({x0, x1}), [&n_calls](taylor_adaptive_batch<double> &t) {
                                            ++n_calls;
                                            for (int i = 0; i < 4; ++i) {
                                                CHECK(t.get_state()[i] >= 0 && t.get_state()[i] < 6.29);
                                            }
                                            return true;
                                        }};
    ta.propagate_until(100., kw::callback = scs);
    CHECK(n_calls > 10);
    CHECK(ta.core().get_last_callback_path() == 1);
    for (int lane = 0; lane < 2; ++lane) {
        for (int pend = 0; pend < 2; ++pend) {
            const auto e0 = energy(st0, lane, pend), e1 = energy(ta.get_state(), lane, pend);
            CHECK(std::abs(e1 - e0) <= 1000. * eps * std::abs(e0));
        }
    }
    // The reducer alone: one launch of the fused kernel, the same numbers as the set, the callback handed back with its indices.
    auto tb = make();
    auto [c_out, cb] = tb.propagate_until(100., kw::callback = callback::angle_reducer({x0, x1}));
    CHECK(!c_out);
    CHECK(tb.core().get_last_callback_path() == 3);
    CHECK(value_isa<callback::angle_reducer>(cb));
    CHECK((value_ref<callback::angle_reducer>(cb).get_indices() == std::vector<std::size_t>{0, 1}));
    CHECK(tb.get_state() == ta.get_state());
    CHECK(tb.get_time() == ta.get_time());
    // Failure modes.
    callback::angle_reducer ar;
    CHECK_THROWS(tb.propagate_until(200., kw::callback = ar), invalid_msg);
    CHECK_THROWS(ar(tb), invalid_msg);
    auto tc = make();
    auto cb1 = std::get<1>(tc.propagate_until(20., kw::callback = callback::angle_reducer({x1})));
    auto td = taylor_adaptive_batch<double>{{prime(x0) = x0}, {0.05, 0.06}, 2u};
    CHECK_THROWS(cb1(td), "Inconsistent state detected in angle_reducer: the last index in the indices vector has a value of "
                          "1, but the number of state variables is only 1");
    std::puts("angle_reducer GPU checks OK");
}

int main(int argc, char **argv)
{
    host_checks();
    if (argc > 1 && std::string(argv[1]) == "gpu") {
        gpu_checks();
    }
    return 0;
}
