// step_action: a library-side step callback defined by assignments `state variable <- expression` and an optional stop
// condition. MI355X EXTENSION: the reference has no counterpart - its step callbacks are code of the
// caller's. The sibling of event_action (event_action.hpp) in the step-callback slot of propagate_until() / _for() /
// _grid(): alone or as a member of a callback set it is recognised by type and applied by a generated kernel
// (hy_step_action, one lane per system) over the device-resident state after every sweep, where the loops invoke a host
// step callback - after the bookkeeping of the sweep and after the events of the step; the state is never downloaded.
//
// Semantics:
//   - the expressions may read state variables, par[...], the time and numbers; ALL of them, the condition included,
//     read the state from BEFORE the action ({x <- v, v <- x} swaps); the time is time_hi after the step;
//   - it acts on the systems whose last step had non-zero length (last_h != 0): a system which has reached its final
//     time, or was retired, takes zero-length steps and is left alone (the per-system rule of the fused angle reducer);
//     a direct call follows the same rule - on a fresh integrator it does nothing;
//   - the values written are, bit for bit, those of cfunc(rhs, vars = state variables) for that state, those parameters
//     and that time: the kernel's section comes from detail::emit_order0() on function_decompose() of the right-hand
//     sides plus the condition. They are not checked for finiteness: the next step reports err_nf_state;
//   - Taylor coefficients, last_h, times, cooldowns and the event log are left alone;
//   - stop_when holds for a system when its value c satisfies !(c == 0) (a NaN stops); the assignments of that sweep are
//     applied first, to the stopping system too. batch_semantics 0, 1, 2: the call returns false when the condition holds
//     for any system it acted on - the loop ends as after a host callback which returned false (cb_stop). batch_semantics
//     3, inside a sweep loop: the system is retired alone with the sticky outcome cb_stop, the call returns
//     true and the other systems carry on (tab_core::get_n_stopped_by_action()).
// The checks against the system (std::invalid_argument) are made when the action first meets an integrator - a left-hand
// side which is not a state variable or is repeated, a variable which is not a state variable, a par[i] the integrator
// does not have; the constructor rejects a left-hand side which is not a variable and an object with neither assignments
// nor a condition.
#pragma once

#include <cstddef>
#include <cstdint>
#include <iosfwd>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "expr_section.hpp"
#include "expression.hpp"
#include "kernel_args.hpp"
#include "taylor_adaptive_batch.hpp"

namespace heyoka_amd
{

class step_action
{
    std::vector<std::pair<expression, expression>> m_assignments;
    std::optional<expression> m_stop_when;

public:
    explicit step_action(std::vector<std::pair<expression, expression>> assignments, std::optional<expression> stop_when = {});
    explicit step_action(expression stop_when);

    [[nodiscard]] const std::vector<std::pair<expression, expression>> &get_assignments() const noexcept
    {
        return m_assignments;
    }
    [[nodiscard]] const std::optional<expression> &get_stop_when() const noexcept
    {
        return m_stop_when;
    }
    // "step_action({v: (0.999 * v)}, stop_when=(x > 2))": also the key of the compiled kernel inside an integrator.
    [[nodiscard]] std::string to_string() const;

    // The step-callback protocol (step_callback.hpp; no pre_hook()): applies the action once, false to stop.
    bool operator()(taylor_adaptive_batch<double> &);
    // (The same on the non-template core of the integrator: what the C ABI and the Python binding hold.)
    bool operator()(detail::tab_core &);
};

std::ostream &operator<<(std::ostream &, const step_action &);

namespace detail
{

// An action checked against a system: the section (expr_section.hpp) of its right-hand sides, followed by the condition
// (has_cond: the last output), and the rows of the state it assigns. The checks are those of assignment_rows() and
// make_expr_section().
struct step_action_section : expr_section {
    std::vector<std::uint32_t> rows;
    bool has_cond = false;
};

step_action_section make_step_action_section(const step_action &act, const std::vector<expression> &state_vars,
                                             std::uint32_t n_par);

// HIP source of the module of one action (kernel hy_step_action, one lane per system, 256 lanes per workgroup): the load
// of last_h, then one straight-line section - loads of the state rows it reads, parameters and time, the right-hand
// sides and the condition, the stores, the stop flag.
std::string make_step_action_source(const step_action_section &sec);

} // namespace detail

} // namespace heyoka_amd
