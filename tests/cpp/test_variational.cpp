// Host half of the variational interface through the drop-in headers: the constructor forms of var_ode_sys as the reference's
// call sites write them (test/taylor_adaptive_var.cpp, test/var_ode_sys.cpp of the reference), the contract of the equations,
// the automatic initial conditions and the messages. Without arguments nothing launches a kernel; with the argument "gpu"
// the harmonic oscillator is propagated and its Taylor map evaluated through the C++ members.
#include <algorithm>
#include <cmath>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <heyoka/expression.hpp>
#include <heyoka/math/cos.hpp>
#include <heyoka/math/sin.hpp>
#include <heyoka/math/time.hpp>
#include <heyoka/taylor.hpp>
#include <heyoka/var_ode_sys.hpp>

using namespace heyoka;

static int failures = 0;

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::cout << "FAILED line " << __LINE__ << ": " #cond << std::endl;                                        \
            ++failures;                                                                                                \
        }                                                                                                              \
    } while (false)

template <typename Ex, typename F>
static void check_throws(int line, const F &f, const std::string &msg)
{
    try {
        f();
    } catch (const Ex &e) {
        if (std::string(e.what()).find(msg) == std::string::npos) {
            std::cout << "FAILED line " << line << ": message '" << e.what() << "' does not contain '" << msg << "'" << std::endl;
            ++failures;
        }
        return;
    } catch (const std::exception &e) {
        std::cout << "FAILED line " << line << ": wrong exception type, message '" << e.what() << "'" << std::endl;
        ++failures;
        return;
    }
    std::cout << "FAILED line " << line << ": nothing was thrown" << std::endl;
    ++failures;
}

// x' = v, v' = -w^2 x with respect to (x0, v0, w) at second order, three systems: the variational variables against their
// closed forms, the map at zero displacement, and the map in w against the solution at w + dw.
static int gpu_half()
{
    auto [x, v] = make_vars("x", "v");
    const auto vsys = var_ode_sys({prime(x) = v, prime(v) = -par[0] * par[0] * x}, {x, v, par[0]}, 2);
    const std::vector<double> x0{1.25, 0.75, 1.}, w{0.9, 1.2, 1.05};
    const std::size_t n = 3;
    auto ta = taylor_adaptive_batch{vsys, {x0[0], x0[1], x0[2], 0., 0., 0.}, 3, kw::pars = w};
    const double t = 12.;
    ta.propagate_until(t);
    const auto st = ta.get_state();
    const double tol = 1e6 * std::ldexp(1., -52);
    for (std::size_t s = 0; s < n; ++s) {
        // Rows: x, v, then dx/d(x0, v0, w) = rows 2 ... 4 and dv/d(x0, v0, w) = rows 5 ... 7.
        CHECK(std::abs(st[0 * n + s] - x0[s] * std::cos(w[s] * t)) <= tol * x0[s]);
        CHECK(std::abs(st[2 * n + s] - std::cos(w[s] * t)) <= tol);
        CHECK(std::abs(st[3 * n + s] - std::sin(w[s] * t) / w[s]) <= tol / w[s]);
        CHECK(std::abs(st[4 * n + s] + x0[s] * t * std::sin(w[s] * t)) <= tol * x0[s] * t);
    }
    const auto &zero = ta.eval_taylor_map(std::vector<double>(3 * n, 0.));
    CHECK(std::equal(zero.begin(), zero.end(), st.begin()));
    CHECK(&zero == &ta.get_tstate());
    const double dw = 1e-3;
    const auto out = ta.eval_taylor_map(std::vector<double>{0., 0., 0., 0., 0., 0., dw, dw, dw});
    for (std::size_t s = 0; s < n; ++s) {
        // Lagrange remainder of the second-order map in w: |x0| (t dw)^3 / 6, plus the integration bound on the terms used.
        const double rem = x0[s] * std::pow(t * dw, 3) / 6 + tol * x0[s] * (1 + t * dw + t * t * dw * dw / 2);
        CHECK(std::abs(out[s] - x0[s] * std::cos((w[s] + dw) * t)) <= rem);
    }
    auto tb = ta;
    CHECK(tb.get_tstate() == ta.get_tstate());
    if (failures != 0) {
        std::cout << failures << " FAILURES" << std::endl;
        return 1;
    }
    std::cout << "GPU OK" << std::endl;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "gpu") {
        return gpu_half();
    }
    auto [x, v] = make_vars("x", "v");

    // The forced damped pendulum of the reference's tests, without the forcing (time-dependent right-hand sides are fine,
    // time as an ARGUMENT is what is refused).
    auto orig_sys = {prime(x) = v, prime(v) = cos(heyoka::time) - par[0] * v - sin(x)};

    // diff() and eval() through the shim.
    {
        CHECK(diff(x * x, x) == 2_dbl * x);
        CHECK(diff(par[0] * x, par[0]) == x);
        CHECK(diff(x, v) == 0_dbl);
        const auto d = diff(sin(x * v), v);
        CHECK(std::abs(eval(d, {{"x", 0.5}, {"v", 2.}}) - 0.5 * std::cos(1.)) < 1e-15);
    }

    // The function kinds which only the decomposition constructs (non-folding sub, div, sum_sq, num_identity): central
    // differences of eval() with the bound of tests/test_variational.py, h^2 |f3| / 6 + eps (|f| + |x f1|) / h, the third
    // derivative f3 from the five-point difference at the step h3, doubled.
    {
        const double h = std::ldexp(1., -17), h3 = std::ldexp(1., -7), eps = std::ldexp(1., -52);
        const std::vector<expression> es{detail::sub(sin(x), x * v), detail::div(x * v, cos(x) + 2_dbl),
                                         detail::sum_sq({x, x * v, sin(x)}), detail::num_identity(expression{1.5}) * x * x,
                                         detail::div(1_dbl, detail::sum_sq({x, v}))};
        for (const auto &e : es) {
            const auto d = diff(e, x);
            for (const double x0 : {0.3, -1.1, 2.5}) {
                const auto f = [&](double t) { return eval(e, {{"x", t}, {"v", 0.75}}); };
                const double xp = x0 + h, xm = x0 - h, fd = (f(xp) - f(xm)) / (xp - xm);
                const double f3 = std::abs(f(x0 + 2 * h3) - 2 * f(x0 + h3) + 2 * f(x0 - h3) - f(x0 - 2 * h3)) / (2 * h3 * h3 * h3);
                const double tol = h * h * 2 * f3 / 6 + eps * (std::abs(f(x0)) + std::abs(x0 * fd)) / h;
                CHECK(std::abs(eval(d, {{"x", x0}, {"v", 0.75}}) - fd) <= tol);
            }
        }
        CHECK(diff(detail::num_identity(expression{3.}), x) == 0_dbl);
        CHECK(diff(heyoka::time, x) == 0_dbl);
        CHECK(eval(heyoka::time * x, {{"x", 2.}}, {}, 1.5) == 3.);
    }

    // Constructor forms: enumerator, initializer list, vector, default order.
    {
        auto vsys = var_ode_sys(orig_sys, var_args::vars, 2);
        CHECK(vsys.get_n_orig_sv() == 2u);
        CHECK(vsys.get_order() == 2u);
        CHECK(vsys.get_sys().size() == 12u);
        CHECK(vsys.get_vargs() == (std::vector{x, v}));
        CHECK(vsys.get_sys()[0].second == v);
        CHECK(vsys.get_sys()[2].first == expression{"∂[(0, 1)]x"});
        CHECK(vsys.get_sys()[7].first == expression{"∂[(0, 1), (1, 1)]x"});
        CHECK(vsys.get_didx()[7] == (var_ode_sys::didx_t{0u, {1u, 1u}}));

        auto v2 = var_ode_sys(orig_sys, {v, x}, 2);
        CHECK(v2.get_vargs() == (std::vector{v, x}));
        auto v3 = var_ode_sys(orig_sys, std::vector{par[0], v});
        CHECK(v3.get_order() == 1u);
        CHECK(v3.get_sys().size() == 6u);
        auto v4 = var_ode_sys(orig_sys, var_args::params | var_args::vars, 3);
        CHECK(v4.get_sys().size() == 2u * 20u);
        auto copy = v4;
        CHECK(copy.get_sys().size() == v4.get_sys().size());
    }

    // Messages.
    using ia = std::invalid_argument;
    check_throws<ia>(__LINE__, [&] { (void)var_ode_sys(orig_sys, var_args::vars, 0); },
                     "The 'order' argument to the var_ode_sys constructor must be nonzero");
    check_throws<ia>(__LINE__, [&] { (void)var_ode_sys(orig_sys, std::vector<expression>{}); },
                     "Cannot formulate the variational equations with respect to an empty list of arguments");
    check_throws<ia>(__LINE__, [&] { (void)var_ode_sys(orig_sys, {x, x}); },
                     "Duplicate entries detected in the list of expressions with respect to which the "
                     "variational equations are to be formulated: [x, x]");
    check_throws<ia>(__LINE__, [&] { (void)var_ode_sys(orig_sys, {x, expression{"z"}}); },
                     "Cannot formulate the variational equations with respect to the "
                     "initial conditions for the variable 'z', which is not among the state variables "
                     "of the system");
    check_throws<ia>(__LINE__, [&] { (void)var_ode_sys(orig_sys, {x + v}); },
                     "the expression is not a variable, not a parameter and not heyoka::time");
    check_throws<ia>(__LINE__, [&] { (void)var_ode_sys({prime(expression{"∂x"}) = v, prime(v) = -expression{"∂x"}}, var_args::vars); },
                     "in a variational ODE system state variable names starting with '∂' are reserved");
    check_throws<not_implemented_error>(__LINE__, [&] { (void)var_ode_sys(orig_sys, var_args::time, 1); }, "initial time");
    check_throws<not_implemented_error>(__LINE__, [&] { (void)var_ode_sys(orig_sys, var_args::all, 1); }, "initial time");
    check_throws<not_implemented_error>(__LINE__, [&] { (void)var_ode_sys(orig_sys, {v, heyoka::time, x}, 1); }, "initial time");

    // Automatic initial conditions (the reference's "auto ic setup batch" cases).
    {
        auto vsys = var_ode_sys(orig_sys, var_args::vars, 2);
        auto ta = taylor_adaptive_batch{vsys, {.2, .21, .3, .31}, 2, kw::tol = 1e-3};
        CHECK(ta.is_variational());
        CHECK(ta.get_vargs() == (std::vector{x, v}));
        CHECK(ta.get_vorder() == 2u);
        CHECK(ta.get_n_orig_sv() == 2u);
        CHECK(ta.get_dim() == 12u);
        const std::vector<double> want{.2, .21, .3, .31, 1, 1, 0, 0, 0, 0, 1, 1};
        CHECK(std::equal(want.begin(), want.end(), ta.get_state().begin()));
        CHECK(std::all_of(ta.get_state().begin() + 12, ta.get_state().end(), [](double val) { return val == 0; }));
        CHECK(ta.get_tstate().size() == 4u);
        std::ostringstream oss;
        oss << ta;
        CHECK(oss.str().find("Variational order") != std::string::npos);
        // Copies keep the variational data.
        auto tb = ta;
        CHECK(tb.is_variational() && tb.get_vorder() == 2u && tb.get_n_orig_sv() == 2u);
        // Wrong input sizes of the map (checked before anything touches the device).
        check_throws<ia>(__LINE__, [&] { ta.eval_taylor_map({1., 2., 3.}); },
                         "Unable to compute the Taylor map: the input range of values has a "
                         "size of 3, which is not a multiple of the batch size 2");
        check_throws<ia>(__LINE__, [&] { ta.eval_taylor_map({1., 2.}); },
                         "Unable to compute the Taylor map: the input range of values has a "
                         "size of 1 (in batches of 2), but the number of variational arguments is 2");
    }
    {
        auto vsys = var_ode_sys(orig_sys, {v, x}, 2);
        auto ta = taylor_adaptive_batch{vsys, {.2, .21, .3, .31}, 2, kw::tol = 1e-3};
        const std::vector<double> want{.2, .21, .3, .31, 0, 0, 1, 1, 1, 1, 0, 0};
        CHECK(std::equal(want.begin(), want.end(), ta.get_state().begin()));
    }
    {
        auto vsys = var_ode_sys(orig_sys, var_args::params, 2);
        auto ta = taylor_adaptive_batch{vsys, {.2, .21, .3, .31}, 2, kw::tol = 1e-3};
        CHECK(ta.get_vargs() == std::vector{par[0]});
        CHECK(std::all_of(ta.get_state().begin() + 4, ta.get_state().end(), [](double val) { return val == 0; }));
    }
    {
        // The full-size state is taken as it is; any other size is the reference's error.
        auto vsys = var_ode_sys(orig_sys, var_args::vars, 1);
        std::vector<double> full(12);
        for (std::size_t i = 0; i < full.size(); ++i) {
            full[i] = 0.5 + static_cast<double>(i);
        }
        auto ta = taylor_adaptive_batch<double>{vsys, full, 2u};
        CHECK(ta.get_state() == full);
        check_throws<ia>(__LINE__, [&] { (void)taylor_adaptive_batch<double>{vsys, std::vector<double>(6), 2u}; },
                         "Inconsistent sizes detected in the initialization of a variational adaptive Taylor "
                         "integrator in batch mode: the state vector has a dimension of 6 (in batches of 2), while the "
                         "total number of equations is 6. The size of the state vector must be "
                         "equal either to the total number of equations times the batch size, or to the number of original "
                         "(i.e., non-variational) equations, which for this system is 2, times the batch size");
    }
    {
        // Non-variational integrators.
        auto ta = taylor_adaptive_batch<double>{{prime(x) = v, prime(v) = -x}, std::vector<double>(4), 2u};
        CHECK(!ta.is_variational());
        CHECK(ta.get_n_orig_sv() == 2u);
        check_throws<ia>(__LINE__, [&] { (void)ta.get_vargs(); },
                         "The function 'get_vargs()' cannot be invoked on non-variational batch integrators");
        check_throws<ia>(__LINE__, [&] { (void)ta.get_vorder(); },
                         "The function 'get_vorder()' cannot be invoked on non-variational batch integrators");
        check_throws<ia>(__LINE__, [&] { (void)ta.get_tstate(); },
                         "The function 'get_tstate()' cannot be invoked on non-variational batch integrators");
        check_throws<ia>(__LINE__, [&] { ta.eval_taylor_map({1., 2.}); },
                         "The function 'eval_taylor_map()' cannot be invoked on non-variational batch integrators");
    }

    if (failures != 0) {
        std::cout << failures << " FAILURES" << std::endl;
        return 1;
    }
    std::cout << "HOST OK" << std::endl;
    return 0;
}
