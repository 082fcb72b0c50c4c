// Ensemble statistics. MI355X EXTENSION. With a list of ensemble statistics next to the observables of
// propagate_grid() the observables are folded ACROSS the systems per grid point. Let Y[g, o, i] be the output of the same call
// with the observables alone (row g, observable o, lane i; NaN where the row was not reached) and V the non-NaN entries of
// Y[g, o, :]. Per (g, o):
//   count      |V| as a double;
//   min / max  the extremum of V in the total order -inf < ... < -0.0 < +0.0 < ... < +inf, NaN if V is empty;
//   sum        the exact real sum of V, rounded once to nearest-even: +0.0 for an exact zero and for an empty V, +-inf beyond the
//              largest double, +inf (-inf) if V holds +inf (-inf), NaN if it holds both;
//   sum_sq     the same over q = y * y, ONE rounded multiplication per value (a q which overflows counts as +inf);
//   mean       sum / count, one division of the two doubles above (NaN if count is 0).
// The result does not depend on the order of the lanes, on the launches in which they reach a row, on the sharding of the
// ensemble: every accumulator is an integer which integer atomics update.
//
// The accumulators are a record of 64-bit words per (g, o) - record (g * n_obs + o) -, holding only what the list needs
// (ens_layout): the counter, the keys of the extrema (hy_ens_key(): the order of the keys as unsigned integers is the total
// order above; all-ones / 0 are the start values of min / max), and per sum a block of ens_sum_words words: ens_n_bins bins of
// weight 2^(32 b - 1074) followed by the counters of +inf and -inf. A finite nonzero double is +-M * 2^(p - 1074) with a 53-bit
// M and p = 0 ... 2045: hy_ens_split() cuts M << (p & 31) into three 32-bit pieces, which are added with the sign to the bins
// (p >> 5), + 1 and + 2. A bin changes by less than 2^32 per value: after up to 2^30 values - over all the records merged into
// one - its magnitude is below 2^62, so an int64 bin cannot overflow. ens_finish() carries the bins into one two's-complement
// integer and rounds its magnitude once.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "kernel_args.hpp"
#include "kw.hpp"

// The text shared by the host (compiled right here) and the emitted module (ens_shared_text()), the way HY_KARGS shares the
// argument blocks. The module defines HY_ENS_FN as __device__ __forceinline__.
#define HY_ENS_FN inline
#define HY_ENS_SHARED(...)                                                                                                     \
    __VA_ARGS__                                                                                                                \
    inline const char *ens_shared_text()                                                                                       \
    {                                                                                                                          \
        return #__VA_ARGS__;                                                                                                   \
    }

namespace heyoka_amd::detail
{

HY_ENS_SHARED(
    // The order-preserving key of the bits of a double which is not NaN.
    HY_ENS_FN u64 hy_ens_key(const u64 bits)
    {
        return (bits >> 63) != 0u ? ~bits : (bits | 0x8000000000000000ull);
    }
    // The bits of a finite nonzero double: M << (p & 31) as three 32-bit pieces, least significant first. Returns the bin
    // p >> 5 of the first piece.
    HY_ENS_FN unsigned hy_ens_split(const u64 bits, unsigned *p0, unsigned *p1, unsigned *p2)
    {
        const unsigned e = (unsigned)(bits >> 52) & 0x7ffu;
        const u64 M = (bits & 0xfffffffffffffull) | (e != 0u ? 0x10000000000000ull : 0ull);
        const unsigned p = e != 0u ? e - 1u : 0u;
        const unsigned sh = p & 31u;
        const u64 t0 = (M & 0xffffffffull) << sh;
        const u64 t1 = (t0 >> 32) + ((M >> 32) << sh);
        *p0 = (unsigned)t0;
        *p1 = (unsigned)t1;
        *p2 = (unsigned)(t1 >> 32);
        return p >> 5;
    }
)

inline constexpr const char *ensemble_statistic_names[] = {"count", "min", "max", "sum", "sum_sq", "mean"};
inline constexpr int n_ensemble_statistics = 6;

inline constexpr std::uint32_t ens_n_bins = 66;
inline constexpr std::uint32_t ens_sum_words = ens_n_bins + 2u;

// The words of a record, by component (-1: not kept). mean keeps sum and count as hidden components.
struct ens_layout {
    int count = -1, min = -1, max = -1, sum = -1, sum_sq = -1;
    std::uint32_t words = 0;
};
ens_layout ens_layout_of(const std::vector<ensemble_statistic> &stats);

// The statistics of a list of codes. std::invalid_argument: an empty list, an unknown code, a statistic named twice.
std::vector<ensemble_statistic> ensemble_statistics_from_codes(const int *codes, std::size_t n);
void check_ensemble_statistics(const std::vector<ensemble_statistic> &stats);
// The messages of grid_sampling.
inline constexpr const char *ensemble_statistics_need_observables
    = "The ensemble statistics of propagate_grid() need a list of observables";
inline constexpr const char *ensemble_statistics_exclude_statistics
    = "The ensemble statistics of propagate_grid() cannot be combined with statistics over the grid";

// n_rec records in their start state.
std::vector<std::uint64_t> ens_init(const ens_layout &l, std::size_t n_rec);
// One value into one record: the host twin of the merge of the emitted module.
void ens_add(const ens_layout &l, std::uint64_t *rec, double y);
// dst += src over n_rec records: integer addition of counters and bins, min / max of the keys.
void ens_merge(const ens_layout &l, std::uint64_t *dst, const std::uint64_t *src, std::size_t n_rec);
// The values of n_rec records, out[rec * stats.size() + k].
void ens_finish(const ens_layout &l, const std::vector<ensemble_statistic> &stats, const std::uint64_t *acc, std::size_t n_rec,
                double *out);

// The device text of the merge of one value into one record for a layout: hy_ens_merge(u64 *rec, double y). aggregate: the
// lanes of a wavefront which merge into the same words are summed in an elected lane first (false: one atomic per lane and
// word, HEYOKA_AMD_GRID_ENS=peratomic - the same words either way).
std::string ens_device_text(const ens_layout &l, bool aggregate);

} // namespace heyoka_amd::detail
