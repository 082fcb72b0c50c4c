// Symbolic differentiation and host-side evaluation. See expression_diff.hpp.
#include "expression_diff.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <set>
#include <stdexcept>

namespace heyoka_amd
{

namespace
{

bool is_zero(const expression &e)
{
    return e.is_number() && e.num() == 0;
}

// Derivative of the function node e, given the derivatives da of its arguments. Everything goes through the folding
// operators: an argument which does not depend on x contributes a 0 which swallows its product and drops out of its sum.
expression diff_node(const expression &e, const std::vector<expression> &da)
{
    const auto &f = e.fn();
    const auto &a = f.args();
    const expression one{1.}, two{2.};

    switch (f.kind()) {
        case func_kind::sum:
            return sum(da);
        case func_kind::prod: {
            // (Equal terms are collected: d(x * x) = 2 * x rather than x + x.)
            std::vector<expression> terms;
            std::vector<double> mult;
            for (std::size_t i = 0; i < a.size(); ++i) {
                if (is_zero(da[i])) {
                    continue;
                }
                auto factors = a;
                factors[i] = da[i];
                auto t = prod(std::move(factors));
                const auto it = std::find(terms.begin(), terms.end(), t);
                if (it == terms.end()) {
                    terms.push_back(std::move(t));
                    mult.push_back(1.);
                } else {
                    mult[static_cast<std::size_t>(it - terms.begin())] += 1.;
                }
            }
            for (std::size_t i = 0; i < terms.size(); ++i) {
                terms[i] = expression{mult[i]} * terms[i];
            }
            return sum(std::move(terms));
        }
        case func_kind::pow: {
            const auto &b = a[0], &ex = a[1];
            if (ex.is_number()) {
                return ex * pow(b, expression{ex.num() - 1.}) * da[0];
            }
            // b^ex (ex' log b + ex b' / b)
            return e * (da[1] * log(b) + ex * da[0] / b);
        }
        case func_kind::sub:
            return da[0] - da[1];
        case func_kind::div:
            return da[0] / a[1] - a[0] * da[1] / (a[1] * a[1]);
        case func_kind::sum_sq: {
            std::vector<expression> terms;
            for (std::size_t i = 0; i < a.size(); ++i) {
                terms.push_back(a[i] * da[i]);
            }
            return two * sum(std::move(terms));
        }
        case func_kind::sin:
            return cos(a[0]) * da[0];
        case func_kind::cos:
            return -sin(a[0]) * da[0];
        case func_kind::exp:
            return e * da[0];
        case func_kind::log:
            return da[0] / a[0];
        case func_kind::time:
        case func_kind::num_identity:
            return expression{0.};
        case func_kind::tan:
            return (one + e * e) * da[0];
        case func_kind::tanh:
            return (one - e * e) * da[0];
        case func_kind::sinh:
            return cosh(a[0]) * da[0];
        case func_kind::cosh:
            return sinh(a[0]) * da[0];
        case func_kind::asin:
            return pow(one - a[0] * a[0], expression{-.5}) * da[0];
        case func_kind::acos:
            return -pow(one - a[0] * a[0], expression{-.5}) * da[0];
        case func_kind::atan:
            return da[0] / (one + a[0] * a[0]);
        case func_kind::asinh:
            return pow(a[0] * a[0] + one, expression{-.5}) * da[0];
        case func_kind::acosh:
            return pow(a[0] * a[0] - one, expression{-.5}) * da[0];
        case func_kind::atanh:
            return da[0] / (one - a[0] * a[0]);
        case func_kind::erf:
            // 2 / sqrt(pi)
            return expression{0x1.20dd750429b6dp+0} * exp(-(a[0] * a[0])) * da[0];
        case func_kind::sigmoid:
            return e * (one - e) * da[0];
        case func_kind::atan2:
            // atan2(y, x): (x y' - y x') / (x^2 + y^2)
            return (a[1] * da[0] - a[0] * da[1]) / (a[1] * a[1] + a[0] * a[0]);
        case func_kind::kepE:
            // E(e, M): dE/de = sin E / (1 - e cos E), dE/dM = 1 / (1 - e cos E).
            return (sin(e) * da[0] + da[1]) / (one - a[0] * cos(e));
        case func_kind::relu:
            return relup(a[0], a[1].num()) * da[0];
        case func_kind::select:
            if (da[1].is_number() && da[2].is_number() && da[1] == da[2]) {
                return da[1];
            }
            return select(a[0], da[1], da[2]);
        case func_kind::relup:
        case func_kind::logical_and:
        case func_kind::logical_or:
        case func_kind::rel_eq:
        case func_kind::rel_neq:
        case func_kind::rel_lt:
        case func_kind::rel_gt:
        case func_kind::rel_lte:
        case func_kind::rel_gte:
            return expression{0.};
        case func_kind::custom:
            break;
    }
    throw not_implemented_error("The derivative of the function '" + f.name()
                                + "' is not available: functions defined through a node rule have no gradient");
}

expression diff_leaf(const expression &l, const expression &x)
{
    return expression{(l == x) ? 1. : 0.};
}

} // namespace

expression diff(ptr_ex_map &cache, const expression &e, const expression &x)
{
    if (!x.is_variable() && !x.is_param()) {
        throw std::invalid_argument("Derivatives are currently supported only with respect to variables and parameters");
    }
    if (!e.is_func()) {
        return diff_leaf(e, x);
    }
    const auto get = [&](const expression &a) { return a.is_func() ? cache.at(a.fn().get_ptr()) : diff_leaf(a, x); };
    // (Arguments before the nodes which use them, every shared node once: no recursion on the depth of the expression.)
    for (const auto *node : function_nodes_postorder(e, [&cache](const void *id) { return cache.count(id) != 0u; })) {
        const auto &args = node->fn().args();
        std::vector<expression> da;
        da.reserve(args.size());
        for (const auto &a : args) {
            da.push_back(get(a));
        }
        cache.emplace(node->fn().get_ptr(), diff_node(*node, da));
    }
    return cache.at(e.fn().get_ptr());
}

expression diff(const expression &e, const expression &x)
{
    ptr_ex_map cache;
    return diff(cache, e, x);
}

namespace
{

// E - e sin E = M by Newton's method from the starter M + e sin M, for 0 <= e < 1 (NaN outside).
double kepE_host(double e, double M)
{
    if (!std::isfinite(e) || !std::isfinite(M) || e < 0 || e >= 1) {
        return std::numeric_limits<double>::quiet_NaN();
    }
    double E = M + e * std::sin(M);
    for (int it = 0; it < 64; ++it) {
        const double fE = E - e * std::sin(E) - M;
        const double dE = fE / (1. - e * std::cos(E));
        E -= dE;
        if (std::abs(dE) <= 4. * std::numeric_limits<double>::epsilon() * std::max(1., std::abs(E))) {
            break;
        }
    }
    return E;
}

struct evaluator {
    const std::unordered_map<std::string, double> &vars;
    const std::vector<double> &pars;
    double time;
    std::unordered_map<const void *, double> memo;

    double leaf(const expression &l) const
    {
        if (l.is_number()) {
            return l.num();
        }
        if (l.is_variable()) {
            const auto it = vars.find(l.var_name());
            if (it == vars.end()) {
                throw std::invalid_argument("Cannot evaluate an expression: no value was provided for the variable '"
                                            + l.var_name() + "'");
            }
            return it->second;
        }
        if (l.par_idx() >= pars.size()) {
            throw std::invalid_argument("Cannot evaluate an expression: the parameter index " + std::to_string(l.par_idx())
                                        + " is out of range (" + std::to_string(pars.size()) + " values were provided)");
        }
        return pars[l.par_idx()];
    }

    double node(const func &f, const std::vector<double> &v) const
    {
        switch (f.kind()) {
            case func_kind::sum: {
                double r = 0;
                for (const auto x : v) {
                    r += x;
                }
                return r;
            }
            case func_kind::prod: {
                double r = 1;
                for (const auto x : v) {
                    r *= x;
                }
                return r;
            }
            case func_kind::pow:
                return std::pow(v[0], v[1]);
            case func_kind::sub:
                return v[0] - v[1];
            case func_kind::div:
                return v[0] / v[1];
            case func_kind::sum_sq: {
                double r = 0;
                for (const auto x : v) {
                    r += x * x;
                }
                return r;
            }
            case func_kind::sin:
                return std::sin(v[0]);
            case func_kind::cos:
                return std::cos(v[0]);
            case func_kind::exp:
                return std::exp(v[0]);
            case func_kind::log:
                return std::log(v[0]);
            case func_kind::time:
                return time;
            case func_kind::num_identity:
                return v[0];
            case func_kind::tan:
                return std::tan(v[0]);
            case func_kind::tanh:
                return std::tanh(v[0]);
            case func_kind::sinh:
                return std::sinh(v[0]);
            case func_kind::cosh:
                return std::cosh(v[0]);
            case func_kind::asin:
                return std::asin(v[0]);
            case func_kind::acos:
                return std::acos(v[0]);
            case func_kind::atan:
                return std::atan(v[0]);
            case func_kind::asinh:
                return std::asinh(v[0]);
            case func_kind::acosh:
                return std::acosh(v[0]);
            case func_kind::atanh:
                return std::atanh(v[0]);
            case func_kind::erf:
                return std::erf(v[0]);
            case func_kind::sigmoid:
                return 1. / (1. + std::exp(-v[0]));
            case func_kind::atan2:
                return std::atan2(v[0], v[1]);
            case func_kind::kepE:
                return kepE_host(v[0], v[1]);
            case func_kind::relu:
                return v[0] > 0 ? v[0] : v[1] * v[0];
            case func_kind::relup:
                return v[0] > 0 ? 1. : v[1];
            case func_kind::select:
                return v[0] != 0 ? v[1] : v[2];
            case func_kind::logical_and: {
                for (const auto x : v) {
                    if (x == 0) {
                        return 0.;
                    }
                }
                return 1.;
            }
            case func_kind::logical_or: {
                for (const auto x : v) {
                    if (x != 0) {
                        return 1.;
                    }
                }
                return 0.;
            }
            case func_kind::rel_eq:
                return v[0] == v[1] ? 1. : 0.;
            case func_kind::rel_neq:
                return v[0] != v[1] ? 1. : 0.;
            case func_kind::rel_lt:
                return v[0] < v[1] ? 1. : 0.;
            case func_kind::rel_gt:
                return v[0] > v[1] ? 1. : 0.;
            case func_kind::rel_lte:
                return v[0] <= v[1] ? 1. : 0.;
            case func_kind::rel_gte:
                return v[0] >= v[1] ? 1. : 0.;
            case func_kind::custom:
                break;
        }
        throw not_implemented_error("Cannot evaluate the function '" + f.name()
                                    + "' on the host: functions defined through a node rule exist only as device code");
    }

    double run(const expression &e)
    {
        if (!e.is_func()) {
            return leaf(e);
        }
        for (const auto *n : function_nodes_postorder(e, [this](const void *id) { return memo.count(id) != 0u; })) {
            const auto &f = n->fn();
            std::vector<double> v;
            v.reserve(f.args().size());
            for (const auto &a : f.args()) {
                v.push_back(a.is_func() ? memo.at(a.fn().get_ptr()) : leaf(a));
            }
            memo.emplace(f.get_ptr(), node(f, v));
        }
        return memo.at(e.fn().get_ptr());
    }
};

} // namespace

double eval(const expression &e, const std::unordered_map<std::string, double> &vars, const std::vector<double> &pars,
            double time)
{
    evaluator ev{vars, pars, time, {}};
    return ev.run(e);
}

std::size_t count_function_nodes(const std::vector<expression> &v_ex)
{
    std::set<const void *> seen;
    std::size_t n = 0;
    for (const auto &e : v_ex) {
        n += function_nodes_postorder(e, [&seen](const void *id) { return seen.count(id) != 0u; }).size();
        // (function_nodes_postorder() does not record: mark what this expression contributed.)
        std::vector<const expression *> stack{&e};
        while (!stack.empty()) {
            const auto *cur = stack.back();
            stack.pop_back();
            if (cur->is_func() && seen.insert(cur->fn().get_ptr()).second) {
                for (const auto &a : cur->fn().args()) {
                    stack.push_back(&a);
                }
            }
        }
    }
    return n;
}

} // namespace heyoka_amd
