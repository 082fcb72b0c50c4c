// Ensemble histograms. MI355X EXTENSION. With a list of bin edges per observable next to the observables of
// propagate_grid() the observables are binned ACROSS the systems per grid point. Let Y[g, o, i] be the output of the same call
// with the observables alone (row g, observable o, lane i; NaN where the row was not reached), and E[0] < ... < E[B] the edges of
// observable o. The slot of a value y which is not NaN is s = #{ j : E[j] <= y }, by IEEE comparisons alone
// (numpy.searchsorted(E, y, side="right")): 0 the underflow slot, 1 ... B the bin [E[s - 1], E[s]), B + 1 the overflow slot;
// -0.0 and +0.0 share a slot; a NaN is skipped. There is no floating-point arithmetic in the definition and none in the result.
//
// The record of (g, o) is B + 2 unsigned 64-bit counters in slot order. The records of one grid point follow each other in the
// order of the observables which have edges: hist_layout::words words per grid point, whatever the number of systems. Merging
// is integer addition: the same words for any order of the lanes, either loop of the call, one batch or its merged shards.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace heyoka_amd::detail
{

inline constexpr std::uint32_t hist_max_bins = 4096;

// How the emitted module merges one count into its word (HEYOKA_AMD_GRID_HIST; the same words in every mode).
//   peratomic  one 64-bit atomic add per lane;
//   aggregate  the lanes of a wavefront which count into the same word are counted in an elected lane, group after group,
//              until no lane is left;
//   hybrid     at most hist_hybrid_turns turns of that loop, which take out the words many lanes share; the lanes still
//              left - spread over many words - issue their own atomic.
enum class hist_mode : int { peratomic = 0, aggregate = 1, hybrid = 2 };
inline constexpr const char *hist_mode_names[] = {"peratomic", "aggregate", "hybrid"};
// (1, 2 and 4 were measured; HEYOKA_AMD_GRID_HIST_TURNS=1|2|4 is the switch of that measurement.)
inline constexpr unsigned hist_hybrid_turns = 1;
unsigned hist_turns_from_env();
inline constexpr hist_mode hist_default_mode = hist_mode::hybrid;
// The mode HEYOKA_AMD_GRID_HIST names (unset or empty: the default). std::invalid_argument: any other value.
hist_mode hist_mode_from_env();

// The records of one grid point: per observable the number of bins (0: no histogram), the offset of its record among the
// words of the grid point, the offset of its edges in the table of all edges.
struct hist_layout {
    std::vector<std::uint32_t> bins, off, edge_off;
    std::uint32_t words = 0, n_edges = 0;
};

// The messages of grid_sampling.
inline constexpr const char *ensemble_histograms_need_observables
    = "The ensemble histograms of propagate_grid() need a list of observables";
inline constexpr const char *ensemble_histograms_exclude_statistics
    = "The ensemble histograms of propagate_grid() cannot be combined with statistics over the grid";

// The checks of the lists of edges of n_obs observables (an empty list: no histogram for that observable).
// std::invalid_argument: another number of lists, no edges at all, fewer than 2 edges, edges which are not finite and strictly
// increasing, more than hist_max_bins bins.
void check_ensemble_histograms(const std::vector<std::vector<double>> &edges, std::size_t n_obs);
// The layout of the numbers of edges per observable (0: none), checked as far as the numbers go.
hist_layout hist_layout_of(const std::size_t *n_edges, std::size_t n_obs);
hist_layout hist_layout_of(const std::vector<std::vector<double>> &edges);
// The edges of all observables, one list behind the other (hist_layout::edge_off).
std::vector<double> hist_edge_table(const std::vector<std::vector<double>> &edges);

// The records of n_grid grid points in their start state.
std::vector<std::uint64_t> hist_init(const hist_layout &l, std::size_t n_grid);
// The slot of y among the n_edges edges e: the bin search of the emitted module, step for step. y is not NaN.
std::uint32_t hist_slot(const double *e, std::uint32_t n_edges, double y);
// One value of observable o into the words of its grid point (rec: the first word of the grid point; table: the edge
// table): the host twin of one merge. A NaN and an observable without edges are skipped.
void hist_add(const hist_layout &l, const double *table, std::uint64_t *rec, std::size_t o, double y);
// dst += src over n_grid grid points.
void hist_merge(const hist_layout &l, std::uint64_t *dst, const std::uint64_t *src, std::size_t n_grid);
// The smallest slot of observable o at one grid point (rec: its first word) whose cumulative count reaches the 1-based rank k;
// -1 if k is 0 or larger than the number of values.
std::int64_t hist_rank_slot(const hist_layout &l, const std::uint64_t *rec, std::size_t o, std::uint64_t k);

// The device text of the histograms of a layout: hy_hist_slot() and hy_hist_count(), with `turns` turns of the hybrid mode. with_ens: the records stand behind
// those of the ensemble statistics (HY_ENS_WORDS is defined).
std::string hist_device_text(const hist_layout &l, hist_mode mode, unsigned turns, bool with_ens);
// The statement of the section which searches and merges the value named y of observable o (with edges) at grid point g.
std::string hist_device_call(const hist_layout &l, std::size_t o, const std::string &y);

} // namespace heyoka_amd::detail
