// Grid observables. MI355X EXTENSION: the reference's propagate_grid() returns the whole state at every grid
// point. A list of expressions over the state variables, par[...] and the time, given to propagate_grid(): the output has
// one column per observable - out[(point * n_obs + observable) * N + lane] - instead of one per state variable. The
// post-step kernel of the grid loop (hy_grid_post, make_grid_source()) evaluates the dense output of the state rows the
// observables read, runs the straight-line section of detail::emit_order0() (cfunc.hpp) on them and stores the results:
// a reached row holds, bit for bit, what cfunc(observables, vars = state variables) returns for the state sample of that
// row, the parameters of the lane and the grid time of the row; a row which is not reached is NaN in every column.
//
// Grid statistics: with a list of statistics next to the observables nothing is stored per grid point. Let
// y_g be the value of an observable of a lane at the g-th grid point the lane reaches (g = 0 ... r - 1, a prefix of its grid)
// and t_g the grid time of that row. Every (observable, statistic) is one double per lane, folded in ascending g:
//   min / max   m = y_0; then, if y_g < m (y_g > m) or m != m: m = y_g - NaN values are ignored unless all are NaN, -0.0 does
//               not replace +0.0;
//   t_min / t_max   the grid time at which the current minimum / maximum was first attained;
//   sum         s = y_0, then s = s + y_g, one rounded addition per point (NaN propagates);
//   last        y_{r-1};    count   r as a double.
// With r = 0 (the first grid point was not reached) every statistic is NaN and count is 0. The output is
// out[(observable * n_stat + statistic) * N + lane], statistics in the order of the list. The accumulators are those slots,
// followed by hidden ones (the extremum behind a t_min / t_max which was asked for alone): n_slots * N doubles owned by their
// lanes, read and written by hy_grid_post at every grid point, with a shadow copy of the same size behind them - a sweep
// which merges copies the lane's slots there first, and hy_grid_unsample puts them back where the plain module clears rows.
#pragma once

#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "expr_section.hpp"
#include "expression.hpp"
#include "grid_ensemble.hpp"
#include "grid_histogram.hpp"
#include "kw.hpp"

namespace heyoka_amd::detail
{

// What propagate_grid() samples: nothing but the state (both absent), a list of observables, or the statistics of a list of
// observables. The construction is the one place which rejects statistics without observables
// (grid_statistics_need_observables) and checks the list of statistics (check_grid_statistics()).
// ... or the statistics of a list of observables across the ensemble per grid point (grid_ensemble.hpp): rejected
// here without observables, together with statistics over the grid, and when check_ensemble_statistics() says so.
struct grid_sampling {
    std::optional<std::vector<expression>> observables;
    std::optional<std::vector<grid_statistic>> statistics;
    std::optional<std::vector<ensemble_statistic>> ensemble;
    // ... and / or the histograms of the observables across the ensemble per grid point (grid_histogram.hpp): a
    // list of bin edges per observable, an empty one for none. Rejected here without observables, together with statistics over
    // the grid, and when check_ensemble_histograms() says so.
    std::optional<std::vector<std::vector<double>>> histograms;

    grid_sampling() = default;
    explicit grid_sampling(std::optional<std::vector<expression>> obs, std::optional<std::vector<grid_statistic>> stats = {},
                           std::optional<std::vector<ensemble_statistic>> ens = {},
                           std::optional<std::vector<std::vector<double>>> hist = {});
};

// Observables checked against a system: their section (expr_section.hpp: `reads` are the rows the kernel samples) and how
// the kernel holds the samples of a grid point.
struct grid_obs_section : expr_section {
    std::uint32_t n_obs = 0;
    // false: registers (the rows are named scalars), true: staged (the rows go through hy_grid_args::stage).
    bool staged = false;
    // Grid statistics, empty: none. n_slots: accumulators per lane, the n_obs * stats.size() of the output first.
    std::vector<grid_statistic> stats;
    std::uint32_t n_slots = 0;
    // Ensemble statistics, empty: none. The records of ens_layout, and whether the lanes of a wavefront are aggregated ahead
    // of the atomics (HEYOKA_AMD_GRID_ENS=peratomic: they are not).
    std::vector<ensemble_statistic> ens;
    ens_layout ens_rec;
    bool ens_aggregate = true;
    // Ensemble histograms, hist.words == 0: none. The records of hist_layout - the numbers of bins, not the edges, which are
    // data of the call - and the way of merging (HEYOKA_AMD_GRID_HIST).
    hist_layout hist;
    hist_mode hist_merge_mode = hist_default_mode;
    unsigned hist_turns = hist_hybrid_turns;
    // The module merges into records behind `out` which do not depend on the number of lanes.
    [[nodiscard]] bool merges() const
    {
        return !ens.empty() || hist.words != 0u;
    }
};

// The largest number of rows held in registers: see DESIGN 4.3e for the budget.
inline constexpr std::uint32_t grid_obs_max_register_rows = 64;

// The section of gs.observables, with gs.statistics if there are any. std::invalid_argument for an empty list, a variable
// which is not a state variable, a par[i] beyond n_par. The way of holding the samples follows from the number of rows
// unless HEYOKA_AMD_GRID_OBS=registers|staged says otherwise.
grid_obs_section make_grid_obs_section(const grid_sampling &gs, const std::vector<expression> &state_vars, std::uint32_t n_par);

// make_grid_source() (taylor_adaptive_batch.hpp) with the section: hy_grid_post samples the rows of the section only and
// stores HY_NOUT columns per grid point, hy_grid_unsample clears HY_NOUT columns, hy_grid_obs0 computes row 0 from the
// current state. The other kernels of the module are those of the plain module.
// With statistics in the section: hy_grid_post folds the HY_NOUT values of a grid point into the HY_NSLOT accumulators of
// the lane instead of storing them, hy_grid_obs0 starts the accumulators, hy_grid_unsample puts them back from their shadow
// copy. Without statistics the text is, byte for byte, the one of a section without the field.
// With ensemble statistics in the section: hy_grid_post and hy_grid_obs0 merge the HY_NOUT values of a grid point into the
// records (g * HY_NOUT + o) of HY_ENS_WORDS 64-bit words behind `out`, which do not depend on the number of lanes; there is no
// hy_grid_unsample - the host keeps a copy of the records where samples may be taken back.
// With ensemble histograms in the section, alone or behind ensemble statistics: the same two kernels search the slot of every
// value of an observable with edges and count it into the HY_HIST_W words of the grid point, which stand behind the records of
// the ensemble statistics of all grid points; the shadow copy of both and the edge tables follow (grid_histogram.hpp).
std::string make_grid_source(std::uint32_t order, std::uint32_t dim, bool high_accuracy, const grid_obs_section *sec);

// The key of the module of gs (with observables) inside an integrator: the text of the observables, the way of holding the
// samples and the statistics (over the grid, or across the ensemble with the way of merging, HEYOKA_AMD_GRID_ENS), the numbers
// of bins of the histograms - not their edges - and their way of merging (HEYOKA_AMD_GRID_HIST).
std::string grid_obs_key(const grid_sampling &gs);

// ---- grid statistics ----
inline constexpr const char *grid_statistic_names[] = {"min", "max", "t_min", "t_max", "sum", "last", "count"};
inline constexpr int n_grid_statistics = 7;

// The statistics of a list of codes. std::invalid_argument: an empty list, an unknown code, a statistic named twice.
std::vector<grid_statistic> grid_statistics_from_codes(const int *codes, std::size_t n);
// The same checks on a list which is already typed (an enumerator may have been cast from anything).
void check_grid_statistics(const std::vector<grid_statistic> &stats);
// The message of grid_sampling for statistics without observables.
inline constexpr const char *grid_statistics_need_observables = "The statistics of propagate_grid() need a list of observables";

} // namespace heyoka_amd::detail
