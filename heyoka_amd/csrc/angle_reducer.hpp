// callback::angle_reducer: the step callback which keeps angular state variables in [0, 2 pi).
//
// Mirrors the interface of the reference's callback::angle_reducer (include/heyoka/callback/angle_reducer.hpp:51-116,
// src/callback/angle_reducer.cpp:126-316): constructed from a range or an initializer list of variables, pre_hook() looks
// the variables up in the system of the integrator, the call operator applies x -= 2 pi floor(x / 2 pi) to them for
// every element of the batch. From-scratch implementation for the MI355X: the reduction runs on the device - kernel
// hy_angle_reduce over the device-resident state, or, when the reducer is the only step callback of propagate_until() /
// propagate_for(), inside the propagate kernel itself - and never moves the state to the host.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <iosfwd>
#include <memory>
#include <ranges>
#include <type_traits>
#include <utility>
#include <vector>

#include "expression.hpp"
#include "taylor_adaptive_batch.hpp"

namespace heyoka_amd
{

namespace callback
{

class angle_reducer
{
    // Names of the variables to reduce and, once pre_hook() has run, their positions in the system of that integrator.
    // An empty pointer marks the default-constructed / moved-from state.
    struct data;
    std::unique_ptr<data> m_data;

    // The one constructor which does the work: every public constructor converts its elements to expressions and ends here.
    struct from_expressions {
    };
    angle_reducer(from_expressions, const std::vector<expression> &);

    template <typename Range>
    static std::vector<expression> to_expressions(Range &&r)
    {
        std::vector<expression> out;
        for (auto &&elem : r) {
            out.push_back(expression(elem));
        }
        return out;
    }

public:
    // Default construction: an object which can only be copied, assigned to, streamed or destroyed.
    angle_reducer() noexcept;
    ~angle_reducer();
    angle_reducer(const angle_reducer &);
    angle_reducer(angle_reducer &&) noexcept;
    angle_reducer &operator=(const angle_reducer &);
    angle_reducer &operator=(angle_reducer &&) noexcept;

    // From a range or an initializer list of anything an expression can be built from (expressions, names).
    template <std::ranges::input_range Range>
        requires(!std::is_same_v<std::remove_cvref_t<Range>, angle_reducer>)
                && std::is_constructible_v<expression, std::ranges::range_reference_t<Range>>
    explicit angle_reducer(Range &&r) : angle_reducer(from_expressions{}, to_expressions(r))
    {
    }
    template <typename Elem>
        requires std::is_constructible_v<expression, const Elem &>
    angle_reducer(std::initializer_list<Elem> l) : angle_reducer(from_expressions{}, to_expressions(l))
    {
    }

    // The step-callback protocol (step_callback.hpp). pre_hook() rebuilds the sorted list of the indices of the state
    // variables to reduce from ta.get_sys(); the call operator reduces them on the device and returns true.
    void pre_hook(taylor_adaptive_batch<double> &);
    bool operator()(taylor_adaptive_batch<double> &);
    // (The same on the non-template core of the integrator: what the C ABI and the Python binding hold.)
    void pre_hook(detail::tab_core &);
    bool operator()(detail::tab_core &);

    // MI355X extension: false for a default-constructed or moved-from object; the indices set by the last pre_hook().
    [[nodiscard]] bool is_valid() const noexcept;
    [[nodiscard]] const std::vector<std::size_t> &get_indices() const;

    friend std::ostream &operator<<(std::ostream &, const angle_reducer &);
};

std::ostream &operator<<(std::ostream &, const angle_reducer &);

} // namespace callback

} // namespace heyoka_amd
