// Variational ODE systems. See var_ode_sys.hpp.
#include "var_ode_sys.hpp"

#include <algorithm>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>

#include "decompose.hpp"
#include "expression_diff.hpp"

namespace heyoka_amd
{

var_args operator|(var_args a1, var_args a2) noexcept
{
    return var_args{static_cast<unsigned>(a1) | static_cast<unsigned>(a2)};
}

bool operator&(var_args a1, var_args a2) noexcept
{
    return static_cast<bool>(static_cast<unsigned>(a1) & static_cast<unsigned>(a2));
}

struct var_ode_sys::impl {
    sys_t sys;
    std::vector<expression> vargs;
    std::vector<didx_t> didx;
    std::uint32_t n_orig_sv = 0;
    std::uint32_t order = 0;
};

namespace
{

[[noreturn]] void throw_time_arg()
{
    throw not_implemented_error("Variational equations with respect to the initial time (var_args::time, var_args::all or "
                                "heyoka::time in the list of arguments) are not implemented");
}

// The sorted list of the parameter indices appearing in v_ex.
std::vector<std::uint32_t> param_indices(const std::vector<expression> &v_ex)
{
    std::set<std::uint32_t> idx;
    std::unordered_set<const void *> seen;
    std::vector<const expression *> stack;
    for (const auto &e : v_ex) {
        stack.push_back(&e);
    }
    while (!stack.empty()) {
        const auto *cur = stack.back();
        stack.pop_back();
        if (cur->is_param()) {
            idx.insert(cur->par_idx());
        } else if (cur->is_func() && seen.insert(cur->fn().get_ptr()).second) {
            for (const auto &a : cur->fn().args()) {
                stack.push_back(&a);
            }
        }
    }
    return {idx.begin(), idx.end()};
}

// "∂[(0, 1), (2, 1)]x": the sparse list of (argument index, order) pairs in the reference's printed form.
std::string var_name_of(const std::vector<std::uint32_t> &alpha, const std::string &sv_name)
{
    std::string s = "∂[";
    bool first = true;
    for (std::size_t j = 0; j < alpha.size(); ++j) {
        if (alpha[j] != 0u) {
            s += (first ? "(" : ", (") + std::to_string(j) + ", " + std::to_string(alpha[j]) + ")";
            first = false;
        }
    }
    return s + "]" + sv_name;
}

std::string list_to_string(const std::vector<expression> &v)
{
    std::string s = "[";
    for (std::size_t i = 0; i < v.size(); ++i) {
        s += (i == 0u ? "" : ", ") + v[i].to_string();
    }
    return s + "]";
}

} // namespace

namespace detail
{

namespace
{

void multi_indices_rec(std::vector<std::vector<std::uint32_t>> &out, std::vector<std::uint32_t> &cur, std::size_t pos,
                       std::uint32_t left)
{
    if (pos + 1u == cur.size()) {
        cur[pos] = left;
        out.push_back(cur);
        return;
    }
    for (std::uint32_t v = left + 1u; v-- > 0u;) {
        cur[pos] = v;
        multi_indices_rec(out, cur, pos + 1u, left - v);
    }
}

} // namespace

std::vector<std::vector<std::uint32_t>> multi_indices_of_order(std::size_t n_args, std::uint32_t order)
{
    std::vector<std::vector<std::uint32_t>> out;
    if (n_args != 0u) {
        std::vector<std::uint32_t> cur(n_args, 0u);
        multi_indices_rec(out, cur, 0, order);
    }
    return out;
}

} // namespace detail

var_ode_sys::var_ode_sys() noexcept = default;

var_ode_sys::var_ode_sys(const sys_t &sys, std::initializer_list<expression> args, std::uint32_t order)
    : var_ode_sys(sys, std::vector<expression>(args), order)
{
}

var_ode_sys::var_ode_sys(const sys_t &sys, const std::variant<var_args, std::vector<expression>> &args, std::uint32_t order)
{
    validate_ode_sys(sys);

    if (order == 0u) {
        throw std::invalid_argument("The 'order' argument to the var_ode_sys constructor must be nonzero");
    }

    const auto n_sv = static_cast<std::uint32_t>(sys.size());
    std::unordered_map<std::string, std::uint32_t> sv_index;
    std::vector<expression> sys_rhs;
    for (std::uint32_t i = 0; i < n_sv; ++i) {
        const auto &name = sys[i].first.var_name();
        if (name.rfind("∂", 0) == 0u) {
            throw std::invalid_argument("Invalid state variable '" + name
                                        + "' detected: in a variational ODE system "
                                          "state variable names starting with '∂' are reserved");
        }
        sv_index.emplace(name, i);
        sys_rhs.push_back(sys[i].second);
    }

    // The arguments: the initial condition of a state variable (is_par false, idx its position) or a parameter.
    struct arg {
        bool is_par;
        std::uint32_t idx;
    };
    std::vector<arg> vargs;
    std::vector<expression> vargs_hr;

    if (const auto *va_ptr = std::get_if<var_args>(&args)) {
        const auto va = *va_ptr;
        if (va == var_args{0} || va > var_args::all) {
            throw std::invalid_argument("Invalid var_args enumerator detected: the value of the enumerator "
                                        "must be in the [1, 7] range, but a value of "
                                        + std::to_string(static_cast<unsigned>(va)) + " was detected instead");
        }
        if (va & var_args::time) {
            throw_time_arg();
        }
        if (va & var_args::vars) {
            for (std::uint32_t i = 0; i < n_sv; ++i) {
                vargs.push_back({false, i});
                vargs_hr.push_back(sys[i].first);
            }
        }
        if (va & var_args::params) {
            for (const auto p : param_indices(sys_rhs)) {
                vargs.push_back({true, p});
                vargs_hr.push_back(par[p]);
            }
        }
    } else {
        const auto &va = std::get<std::vector<expression>>(args);
        if (va.empty()) {
            throw std::invalid_argument(
                "Cannot formulate the variational equations with respect to an empty list of arguments");
        }
        for (const auto &ex : va) {
            if (ex.is_variable()) {
                const auto it = sv_index.find(ex.var_name());
                if (it == sv_index.end()) {
                    throw std::invalid_argument("Cannot formulate the variational equations with respect to the "
                                                "initial conditions for the variable '"
                                                + ex.var_name()
                                                + "', which is not among the state variables "
                                                  "of the system");
                }
                vargs.push_back({false, it->second});
            } else if (ex.is_param()) {
                // (A parameter which does not appear in the system is allowed, as in the reference: zero equations.)
                vargs.push_back({true, ex.par_idx()});
            } else if (ex == heyoka_amd::time) {
                throw_time_arg();
            } else {
                throw std::invalid_argument("Cannot formulate the variational equations with respect to the expression '"
                                            + ex.to_string()
                                            + "': the "
                                              "expression is not a variable, not a parameter and not heyoka::time");
            }
            vargs_hr.push_back(ex);
        }
        std::unordered_set<expression, expression_hash> uniq(vargs_hr.begin(), vargs_hr.end());
        if (uniq.size() != vargs_hr.size()) {
            throw std::invalid_argument("Duplicate entries detected in the list of expressions with respect to which the "
                                        "variational equations are to be formulated: "
                                        + list_to_string(va));
        }
    }

    const auto n_args = vargs.size();

    auto d = std::make_shared<impl>();
    d->n_orig_sv = n_sv;
    d->order = order;
    d->vargs = vargs_hr;

    // Order 0: the original equations, unchanged.
    for (std::uint32_t i = 0; i < n_sv; ++i) {
        d->sys.push_back(sys[i]);
        d->didx.emplace_back(i, std::vector<std::uint32_t>(n_args, 0u));
    }
    if (n_args == 0u) {
        // (var_args::params on a system without parameters: nothing to differentiate with respect to.)
        m_impl = std::move(d);
        return;
    }

    // Every variable known so far: name -> (component, multi-index), in equation order.
    std::map<std::string, std::size_t> eq_of_name;
    for (std::uint32_t i = 0; i < n_sv; ++i) {
        eq_of_name.emplace(sys[i].first.var_name(), i);
    }

    // The equations of order k from those of order k - 1: with alpha = beta + e_j, j the highest non-zero index of alpha,
    //   rhs(i, alpha) = D_j rhs(i, beta),   D_j g = sum_u (dg/du) D_j u + dg/dpar_j,
    // where u runs over the variables of g - D_j of the variable (l, gamma) is the variable (l, gamma + e_j) - and the last
    // term is there when argument j is a parameter.
    std::size_t prev_begin = 0, prev_end = n_sv;
    for (std::uint32_t k = 1; k <= order; ++k) {
        std::vector<expression> prev_rhs;
        std::map<std::pair<std::uint32_t, std::vector<std::uint32_t>>, std::size_t> prev_pos;
        for (auto e = prev_begin; e < prev_end; ++e) {
            prev_pos.emplace(d->didx[e], prev_rhs.size());
            prev_rhs.push_back(d->sys[e].second);
        }

        // Partial derivatives of the previous right-hand sides: with respect to each variable they contain (one cache per
        // variable, shared by all of them), and with respect to the parameters among the arguments.
        const auto present = get_variables(prev_rhs);
        const std::unordered_set<std::string> present_set(present.begin(), present.end());
        struct partial {
            std::size_t eq; // equation of the variable u (npos: a parameter)
            std::vector<expression> dg;
        };
        std::vector<partial> wrt_vars;
        for (std::size_t e = 0; e < prev_end; ++e) {
            const auto &name = d->sys[e].first.var_name();
            if (present_set.count(name) == 0u) {
                continue;
            }
            partial p{e, {}};
            ptr_ex_map cache;
            for (const auto &g : prev_rhs) {
                p.dg.push_back(diff(cache, g, d->sys[e].first));
            }
            wrt_vars.push_back(std::move(p));
        }
        std::vector<std::vector<expression>> wrt_par(n_args);
        for (std::size_t j = 0; j < n_args; ++j) {
            if (vargs[j].is_par) {
                ptr_ex_map cache;
                for (const auto &g : prev_rhs) {
                    wrt_par[j].push_back(diff(cache, g, par[vargs[j].idx]));
                }
            }
        }

        const auto alphas = detail::multi_indices_of_order(n_args, k);

        // The variables of order k exist before their equations are written (an equation may refer to any of them).
        const auto new_begin = d->sys.size();
        for (std::uint32_t i = 0; i < n_sv; ++i) {
            for (const auto &alpha : alphas) {
                auto name = var_name_of(alpha, sys[i].first.var_name());
                eq_of_name.emplace(name, d->sys.size());
                d->sys.emplace_back(expression{std::move(name)}, expression{0.});
                d->didx.emplace_back(i, alpha);
            }
        }

        for (auto e = new_begin; e < d->sys.size(); ++e) {
            const auto &[comp, alpha] = d->didx[e];
            std::size_t j = n_args - 1u;
            while (alpha[j] == 0u) {
                --j;
            }
            auto beta = alpha;
            --beta[j];
            const auto g = prev_pos.at({comp, beta});

            std::vector<expression> terms;
            for (const auto &p : wrt_vars) {
                const auto &dg = p.dg[g];
                if (dg.is_number() && dg.num() == 0) {
                    continue;
                }
                // D_j u.
                const auto &[ucomp, ugamma] = d->didx[p.eq];
                auto gamma = ugamma;
                ++gamma[j];
                const auto &du = d->sys[eq_of_name.at(var_name_of(gamma, sys[ucomp].first.var_name()))].first;
                terms.push_back(dg * du);
            }
            if (vargs[j].is_par) {
                terms.push_back(wrt_par[j][g]);
            }
            d->sys[e].second = sum(std::move(terms));
        }

        prev_begin = new_begin;
        prev_end = d->sys.size();
    }

    m_impl = std::move(d);
}

var_ode_sys::var_ode_sys(const var_ode_sys &) noexcept = default;
var_ode_sys::var_ode_sys(var_ode_sys &&) noexcept = default;
var_ode_sys &var_ode_sys::operator=(const var_ode_sys &) noexcept = default;
var_ode_sys &var_ode_sys::operator=(var_ode_sys &&) noexcept = default;
var_ode_sys::~var_ode_sys() = default;

const var_ode_sys::sys_t &var_ode_sys::get_sys() const noexcept
{
    return m_impl->sys;
}

const std::vector<expression> &var_ode_sys::get_vargs() const noexcept
{
    return m_impl->vargs;
}

std::uint32_t var_ode_sys::get_n_orig_sv() const noexcept
{
    return m_impl->n_orig_sv;
}

std::uint32_t var_ode_sys::get_order() const noexcept
{
    return m_impl->order;
}

const std::vector<var_ode_sys::didx_t> &var_ode_sys::get_didx() const noexcept
{
    return m_impl->didx;
}

} // namespace heyoka_amd
