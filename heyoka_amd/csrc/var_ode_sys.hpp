// Variational ODE systems: the original equations augmented with the equations of the partial derivatives of the state
// with respect to initial conditions and parameters, up to a given order.
//
// Mirrors the observable contract of the reference's var_ode_sys (include/heyoka/var_ode_sys.hpp:29-75,
// src/var_ode_sys.cpp:215-407): the first get_n_orig_sv() equations are the original ones; then one variational variable per
// (component, multi-index) with symmetric derivatives stored once, sorted by total order, then component, then reverse-
// lexicographic multi-index (src/dtens.cpp:146-160); named "∂" + sparse index list + name of the state variable.
// The construction is this project's own: the total-derivative operator with respect to one argument is applied to the
// right-hand sides of the previous order (expression_diff.hpp), there are no implicit-function placeholders and no
// derivative tensors.
//
// Time as a variational argument (var_args::time, var_args::all, an explicit heyoka::time) is not implemented:
// not_implemented_error.
#pragma once

#include <cstdint>
#include <initializer_list>
#include <memory>
#include <utility>
#include <variant>
#include <vector>

#include "expression.hpp"

namespace heyoka_amd
{

// NOLINTNEXTLINE(performance-enum-size)
enum class var_args : unsigned { vars = 0b001, params = 0b010, time = 0b100, all = 0b111 };

[[nodiscard]] var_args operator|(var_args, var_args) noexcept;
[[nodiscard]] bool operator&(var_args, var_args) noexcept;

namespace detail
{

// The multi-indices over n_args arguments of total order `order`, in the order of the equations (descending lexicographic =
// the reference's reverse-lexicographic comparison, src/dtens.cpp:146-160). The ONE enumeration: var_ode_sys numbers its
// equations with it and the Taylor-map kernels address the state rows with it (taylor_map.hpp).
std::vector<std::vector<std::uint32_t>> multi_indices_of_order(std::size_t n_args, std::uint32_t order);

} // namespace detail

class var_ode_sys
{
    struct impl;
    std::shared_ptr<const impl> m_impl;

public:
    using sys_t = std::vector<std::pair<expression, expression>>;
    // (component, dense multi-index over the variational arguments) of one equation.
    using didx_t = std::pair<std::uint32_t, std::vector<std::uint32_t>>;

    var_ode_sys() noexcept;
    explicit var_ode_sys(const sys_t &, const std::variant<var_args, std::vector<expression>> &, std::uint32_t = 1);
    explicit var_ode_sys(const sys_t &, std::initializer_list<expression>, std::uint32_t = 1);
    var_ode_sys(const var_ode_sys &) noexcept;
    var_ode_sys(var_ode_sys &&) noexcept;
    var_ode_sys &operator=(const var_ode_sys &) noexcept;
    var_ode_sys &operator=(var_ode_sys &&) noexcept;
    ~var_ode_sys();

    [[nodiscard]] const sys_t &get_sys() const noexcept;
    [[nodiscard]] const std::vector<expression> &get_vargs() const noexcept;
    [[nodiscard]] std::uint32_t get_n_orig_sv() const noexcept;
    [[nodiscard]] std::uint32_t get_order() const noexcept;
    // One entry per equation of get_sys(), in its order.
    [[nodiscard]] const std::vector<didx_t> &get_didx() const noexcept;
    [[nodiscard]] bool is_valid() const noexcept
    {
        return static_cast<bool>(m_impl);
    }
};

} // namespace heyoka_amd
