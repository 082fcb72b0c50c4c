// Event-log observables. MI355X EXTENSION: a row of the event log of the recording callbacks
// (event_detection.hpp) holds the whole state at the trigger time behind its header. With a list of expressions over the
// state variables, par[...] and the time set on the integrator, a row holds one column per observable instead:
// 8 + n_obs doubles. The kernel hy_obs_rows takes the place of hy_dout_rows (hip_emit.hpp): one thread per row, the same
// guards, the dense output of the state rows the observables read ONLY - operation by operation the recurrence of
// hy_dout_rows, or the copy of the state after the step for a terminal row -, then the straight-line section of
// detail::emit_order0() (cfunc.hpp) on those samples. Column 8 + k holds, bit for bit, what
// cfunc(observables, vars = state variables) returns for the state columns the same run logs without observables, the
// parameters of the row's system and time = column 4.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "decompose.hpp"
#include "expr_section.hpp"
#include "expression.hpp"
#include "hip_emit.hpp"

namespace heyoka_amd::detail
{

// Observables checked against a system: their section (expr_section.hpp: `reads` are the rows the kernel samples) and how
// the kernel holds the samples of a row of the log.
struct event_obs_section : expr_section {
    std::uint32_t n_obs = 0;
    // false: registers (the rows are named scalars), true: staged (the rows go through hy_drow_args::stage).
    bool staged = false;
};

// std::invalid_argument for an empty list, a variable which is not a state variable, a par[i] beyond n_par, an invalid value
// of HEYOKA_AMD_EVENT_OBS. The way of holding the samples follows from the number of rows read (registers up to
// grid_obs_max_register_rows) unless HEYOKA_AMD_EVENT_OBS=registers|staged says otherwise.
event_obs_section make_event_obs_section(const std::vector<expression> &obs, const std::vector<expression> &state_vars,
                                         std::uint32_t n_par);

// The module of hy_obs_rows for the system prog and the layout of its Taylor coefficients (opts.order, high_accuracy,
// compact_tc, exact_division - the options of make_event_log_dout_source()). Staged mode: the samples of row r of the step
// are stage[j * n_max + r], j the position in section.reads - n_reads * n_max doubles, the row index fastest.
std::string make_event_log_obs_source(const taylor_program &prog, const emit_options &opts, const event_obs_section &section);

} // namespace heyoka_amd::detail
