// Expression sections: what terminal-event actions (event_action.hpp), step actions (step_action.hpp) and grid observables
// (grid_observables.hpp) have in common. A list of expressions over the state variables, par[...] and the time is checked
// against a system and decomposed as a function of ALL the state variables; detail::emit_order0() (cfunc.hpp) turns the
// program into the straight-line device code of the feature's kernel.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "decompose.hpp"
#include "expression.hpp"

namespace heyoka_amd::detail
{

struct expr_section {
    taylor_program prog;
    // The state rows the section reads, sorted: the operands of its elementary functions and the outputs which are plain
    // copies of a row.
    std::vector<std::uint32_t> reads;
};

// The wording of a feature's std::invalid_argument messages.
struct section_wording {
    // Expression k uses the variable v, which is not a state variable of the system.
    std::function<std::string(std::size_t k, const std::string &v)> foreign_variable;
    // The expressions use par[i], but there are n_par parameters.
    std::function<std::string(std::uint32_t i, std::uint32_t n_par)> par_out_of_range;
};

// The checks, in this order: no expression uses a variable which is not in state_vars; function_decompose() and
// make_program(); no par[i] beyond n_par (the kernels index the integrator's parameter array).
expr_section make_expr_section(const std::vector<expression> &fn, const std::vector<expression> &state_vars, std::uint32_t n_par,
                               const section_wording &w);

// The rows of the state a list of assignments `state variable <- expression` writes, in the order of the list.
// std::invalid_argument, assignment by assignment: the left-hand side is not a state variable, the row was assigned already,
// the right-hand side (expression k of the section, k the position in the list) uses a variable which is not a state
// variable. kind: "an event action"; where ends the messages: " (terminal event 2)".
std::vector<std::uint32_t> assignment_rows(const std::vector<std::pair<expression, expression>> &assignments,
                                           const std::vector<expression> &state_vars, const section_wording &w,
                                           const std::string &kind, const std::string &where = {});

// The state variables of a system, in order.
std::vector<expression> state_variables_of(const std::vector<std::pair<expression, expression>> &sys);

} // namespace heyoka_amd::detail
