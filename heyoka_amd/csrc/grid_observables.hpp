// Grid observables. MI355X EXTENSION: the reference's propagate_grid() returns the whole state at every grid
// point. A list of expressions over the state variables, par[...] and the time, given to propagate_grid(): the output has
// one column per observable - out[(point * n_obs + observable) * N + lane] - instead of one per state variable. The
// post-step kernel of the grid loop (hy_grid_post, make_grid_source()) evaluates the dense output of the state rows the
// observables read, runs the straight-line section of detail::emit_order0() (cfunc.hpp) on them and stores the results:
// a reached row holds, bit for bit, what cfunc(observables, vars = state variables) returns for the state sample of that
// row, the parameters of the lane and the grid time of the row; a row which is not reached is NaN in every column.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "decompose.hpp"
#include "expression.hpp"

namespace heyoka_amd::detail
{

// Observables checked against a system: the state rows they read (sorted), their decomposition as a function of ALL the
// state variables, and how the kernel holds the samples of a grid point.
struct grid_obs_section {
    std::vector<std::uint32_t> rows;
    std::uint32_t n_obs = 0;
    // false: registers (the rows are named scalars), true: staged (the rows go through hy_grid_args::stage).
    bool staged = false;
    taylor_program prog;
};

// The largest number of rows held in registers: see DESIGN 4.3e for the budget.
inline constexpr std::uint32_t grid_obs_max_register_rows = 64;

// std::invalid_argument for an empty list, a variable which is not a state variable, a par[i] beyond n_par. The way of
// holding the samples follows from the number of rows unless HEYOKA_AMD_GRID_OBS=registers|staged says otherwise.
grid_obs_section make_grid_obs_section(const std::vector<expression> &obs, const std::vector<expression> &state_vars,
                                       std::uint32_t n_par);

// make_grid_source() (taylor_adaptive_batch.hpp) with the section: hy_grid_post samples the rows of the section only and
// stores HY_NOUT columns per grid point, hy_grid_unsample clears HY_NOUT columns, hy_grid_obs0 computes row 0 from the
// current state. The other kernels of the module are those of the plain module.
std::string make_grid_source(std::uint32_t order, std::uint32_t dim, bool high_accuracy, const grid_obs_section *sec);

// The key of the module of a list of observables inside an integrator: their text and the way of holding the samples.
std::string grid_obs_key(const std::vector<expression> &obs);

} // namespace heyoka_amd::detail
