// Ensemble statistics: the host side of the accumulators and the device text of the merge.
#include "grid_ensemble.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <set>
#include <sstream>
#include <stdexcept>

namespace heyoka_amd::detail
{

void check_ensemble_statistics(const std::vector<ensemble_statistic> &stats)
{
    if (stats.empty()) {
        throw std::invalid_argument("The list of ensemble statistics of propagate_grid() is empty");
    }
    std::set<int> seen;
    for (const auto s : stats) {
        const auto code = static_cast<int>(s);
        if (code < 0 || code >= n_ensemble_statistics) {
            throw std::invalid_argument("The ensemble statistic code " + std::to_string(code) + " of propagate_grid() is unknown");
        }
        if (!seen.insert(code).second) {
            throw std::invalid_argument(std::string("The ensemble statistic '") + ensemble_statistic_names[code]
                                        + "' of propagate_grid() is named twice");
        }
    }
}

std::vector<ensemble_statistic> ensemble_statistics_from_codes(const int *codes, std::size_t n)
{
    std::vector<ensemble_statistic> ret;
    for (std::size_t k = 0; k < n; ++k) {
        ret.push_back(static_cast<ensemble_statistic>(codes[k]));
    }
    check_ensemble_statistics(ret);
    return ret;
}

ens_layout ens_layout_of(const std::vector<ensemble_statistic> &stats)
{
    const auto has = [&](ensemble_statistic s) { return std::find(stats.begin(), stats.end(), s) != stats.end(); };
    const bool mean = has(ensemble_statistic::mean);
    ens_layout l;
    const auto take = [&](bool wanted, int &off, std::uint32_t n) {
        if (wanted) {
            off = static_cast<int>(l.words);
            l.words += n;
        }
    };
    take(has(ensemble_statistic::count) || mean, l.count, 1u);
    take(has(ensemble_statistic::min), l.min, 1u);
    take(has(ensemble_statistic::max), l.max, 1u);
    take(has(ensemble_statistic::sum) || mean, l.sum, ens_sum_words);
    take(has(ensemble_statistic::sum_sq), l.sum_sq, ens_sum_words);
    return l;
}

std::vector<std::uint64_t> ens_init(const ens_layout &l, std::size_t n_rec)
{
    std::vector<std::uint64_t> ret(n_rec * l.words, 0u);
    if (l.min >= 0) {
        for (std::size_t r = 0; r < n_rec; ++r) {
            ret[r * l.words + static_cast<unsigned>(l.min)] = ~std::uint64_t(0);
        }
    }
    return ret;
}

namespace
{

std::uint64_t bits_of(double y)
{
    std::uint64_t b = 0;
    std::memcpy(&b, &y, sizeof(b));
    return b;
}

double from_bits(std::uint64_t b)
{
    double y = 0;
    std::memcpy(&y, &b, sizeof(y));
    return y;
}

// The words of a sum are int64 in two's complement, kept as the unsigned words of the record: additions wrap alike.
void sum_add(std::uint64_t *blk, double v)
{
    const auto bits = bits_of(v);
    const bool neg = (bits >> 63) != 0u;
    if (std::isinf(v)) {
        blk[ens_n_bins + (neg ? 1u : 0u)] += 1u;
        return;
    }
    if (v == 0.) {
        return;
    }
    unsigned p[3];
    const auto b = hy_ens_split(bits, p, p + 1, p + 2);
    for (unsigned k = 0; k < 3u; ++k) {
        blk[b + k] += neg ? (0u - static_cast<std::uint64_t>(p[k])) : static_cast<std::uint64_t>(p[k]);
    }
}

// The bins carried into one two's-complement integer of 32-bit digits, its magnitude rounded once to nearest-even.
double sum_finish(const std::uint64_t *blk)
{
    const auto n_pinf = blk[ens_n_bins], n_ninf = blk[ens_n_bins + 1u];
    if (n_pinf != 0u || n_ninf != 0u) {
        return (n_pinf != 0u && n_ninf != 0u) ? std::numeric_limits<double>::quiet_NaN()
                                              : (n_pinf != 0u ? 1. : -1.) * std::numeric_limits<double>::infinity();
    }
    // (|bin| < 2^62 and |carry| < 2^31: no overflow. The last carry extends the sign over two more digits.)
    constexpr unsigned nd = ens_n_bins + 2u;
    std::uint32_t dig[nd];
    std::int64_t carry = 0;
    for (unsigned b = 0; b < ens_n_bins; ++b) {
        const auto v = static_cast<std::int64_t>(blk[b]) + carry;
        dig[b] = static_cast<std::uint32_t>(static_cast<std::uint64_t>(v));
        carry = v >> 32;
    }
    dig[ens_n_bins] = static_cast<std::uint32_t>(static_cast<std::uint64_t>(carry));
    dig[ens_n_bins + 1u] = static_cast<std::uint32_t>(static_cast<std::uint64_t>(carry) >> 32);
    const bool neg = carry < 0;
    if (neg) {
        std::uint64_t c = 1;
        for (unsigned b = 0; b < nd; ++b) {
            c += static_cast<std::uint32_t>(~dig[b]);
            dig[b] = static_cast<std::uint32_t>(c);
            c >>= 32;
        }
    }
    int top = -1;
    for (int b = static_cast<int>(nd) - 1; b >= 0 && top < 0; --b) {
        if (dig[b] != 0u) {
            top = b * 32 + 31 - __builtin_clz(dig[b]);
        }
    }
    if (top < 0) {
        return 0.;
    }
    const auto bit = [&](int k) { return (dig[k / 32] >> (k % 32)) & 1u; };
    // The magnitude is mag * 2^-1074. The 53 bits from the top, m, and shift = top - 52 (0: mag itself is the bit pattern,
    // subnormal or of exponent 1). The bit pattern (shift << 52) + m counts the hidden bit of m into the exponent field, and a
    // rounding which carries out of the 53 bits moves to the next binade by itself.
    const int shift = std::max(top - 52, 0);
    std::uint64_t m = 0;
    for (int k = std::min(top, shift + 52); k >= shift; --k) {
        m = (m << 1) | bit(k);
    }
    if (shift > 0) {
        bool sticky = false;
        for (int k = shift - 2; k >= 0 && !sticky; --k) {
            sticky = bit(k) != 0u;
        }
        if (bit(shift - 1) != 0u && (sticky || (m & 1u) != 0u)) {
            ++m;
        }
    }
    const auto pattern = (static_cast<std::uint64_t>(shift) << 52) + m;
    const double mag = (pattern >> 52) >= 0x7ffu ? std::numeric_limits<double>::infinity() : from_bits(pattern);
    return neg ? -mag : mag;
}

double key_value(std::uint64_t key)
{
    return from_bits((key >> 63) != 0u ? (key & 0x7fffffffffffffffull) : ~key);
}

} // namespace

void ens_add(const ens_layout &l, std::uint64_t *rec, double y)
{
    if (y != y) {
        return;
    }
    const std::uint64_t key = hy_ens_key(bits_of(y));
    if (l.count >= 0) {
        rec[l.count] += 1u;
    }
    if (l.min >= 0) {
        rec[l.min] = std::min(rec[l.min], key);
    }
    if (l.max >= 0) {
        rec[l.max] = std::max(rec[l.max], key);
    }
    if (l.sum >= 0) {
        sum_add(rec + l.sum, y);
    }
    if (l.sum_sq >= 0) {
        // (One rounded multiplication: nothing to contract it with.)
        volatile double q = y * y;
        sum_add(rec + l.sum_sq, q);
    }
}

void ens_merge(const ens_layout &l, std::uint64_t *dst, const std::uint64_t *src, std::size_t n_rec)
{
    for (std::size_t r = 0; r < n_rec; ++r, dst += l.words, src += l.words) {
        for (std::uint32_t w = 0; w < l.words; ++w) {
            const auto sw = static_cast<int>(w);
            if (sw == l.min) {
                dst[w] = std::min(dst[w], src[w]);
            } else if (sw == l.max) {
                dst[w] = std::max(dst[w], src[w]);
            } else {
                dst[w] += src[w];
            }
        }
    }
}

void ens_finish(const ens_layout &l, const std::vector<ensemble_statistic> &stats, const std::uint64_t *acc, std::size_t n_rec,
                double *out)
{
    const auto nan = std::numeric_limits<double>::quiet_NaN();
    for (std::size_t r = 0; r < n_rec; ++r, acc += l.words) {
        for (const auto s : stats) {
            double v = nan;
            switch (s) {
                case ensemble_statistic::count:
                    v = static_cast<double>(acc[l.count]);
                    break;
                case ensemble_statistic::min:
                    v = acc[l.min] == ~std::uint64_t(0) ? nan : key_value(acc[l.min]);
                    break;
                case ensemble_statistic::max:
                    v = acc[l.max] == 0u ? nan : key_value(acc[l.max]);
                    break;
                case ensemble_statistic::sum:
                    v = sum_finish(acc + l.sum);
                    break;
                case ensemble_statistic::sum_sq:
                    v = sum_finish(acc + l.sum_sq);
                    break;
                case ensemble_statistic::mean:
                    v = acc[l.count] == 0u ? nan : sum_finish(acc + l.sum) / static_cast<double>(acc[l.count]);
                    break;
            }
            *out++ = v;
        }
    }
}

std::string ens_device_text(const ens_layout &l, bool aggregate)
{
    std::ostringstream src;
    src << "\n// Ensemble statistics (DESIGN 4.3g): record (g * HY_NOUT + o) of HY_ENS_WORDS 64-bit words per grid point and observable,\n"
           "// integer atomics only.\n#define HY_ENS_WORDS "
        << l.words << "u\n#define HY_ENS_NBINS " << ens_n_bins << "u\n#define HY_ENS_AGG " << (aggregate ? 1 : 0)
        << "\n#define HY_ENS_FN __device__ __forceinline__\n"
        << ens_shared_text() << R"HIP(

// The 64-bit value v of lane l (uniform, a lane which is active here).
__device__ __forceinline__ u64 hy_ens_rl64(const u64 v, const unsigned l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)l);
    return ((u64)hi << 32) | lo;
}
)HIP";
    if (l.count >= 0 || l.min >= 0 || l.max >= 0) {
        const std::string cnt = "rec + " + std::to_string(std::max(l.count, 0)) + "u", mn = "rec + " + std::to_string(std::max(l.min, 0)) + "u",
                          mx = "rec + " + std::to_string(std::max(l.max, 0)) + "u";
        src << R"HIP(
// The counter and the keys of the extrema of the record rec, for the lanes with pend set. Aggregated: the lanes whose record is
// the one of the first pending lane are folded in that lane, which issues the atomics; then the next group, until no lane is
// left. Every lane which arrives here takes every turn of the loop (the ballots are uniform); only the lanes of a ballot mask
// are read.
__device__ __forceinline__ void hy_ens_cmm(u64 *rec, bool pend, const u64 key)
{
#if HY_ENS_AGG
    for (;;) {
        const u64 m = __builtin_amdgcn_ballot_w64(pend);
        if (m == 0u) break;
        const unsigned l = (unsigned)__builtin_ctzll(m);
        const bool same = pend && (u64)rec == hy_ens_rl64((u64)rec, l);
        u64 grp = __builtin_amdgcn_ballot_w64(same);
        const bool elected = (threadIdx.x & 63u) == l;
)HIP";
        if (l.count >= 0) {
            src << "        if (elected) atomicAdd(" << cnt << ", (u64)__builtin_popcountll(grp));\n";
        }
        if (l.min >= 0 || l.max >= 0) {
            src << "        u64 kmin = ~0ull, kmax = 0ull;\n        while (grp != 0u) {\n            const unsigned j = "
                   "(unsigned)__builtin_ctzll(grp);\n            grp &= grp - 1u;\n            const u64 kj = hy_ens_rl64(key, j);\n"
                   "            kmin = kj < kmin ? kj : kmin;\n            kmax = kj > kmax ? kj : kmax;\n        }\n";
            if (l.min >= 0) {
                src << "        if (elected) atomicMin(" << mn << ", kmin);\n";
            }
            if (l.max >= 0) {
                src << "        if (elected) atomicMax(" << mx << ", kmax);\n";
            }
        } else {
            src << "        (void)key;\n";
        }
        src << "        pend = pend && !same;\n    }\n#else\n    if (pend) {\n";
        if (l.count >= 0) {
            src << "        atomicAdd(" << cnt << ", 1ull);\n";
        }
        if (l.min >= 0) {
            src << "        atomicMin(" << mn << ", key);\n";
        }
        if (l.max >= 0) {
            src << "        atomicMax(" << mx << ", key);\n";
        }
        src << "    }\n    (void)key;\n#endif\n}\n";
    }
    if (l.sum >= 0 || l.sum_sq >= 0) {
        src << R"HIP(
// The value of the bits v, which is not NaN in the lanes with ok set, into the block blk of a sum: an infinity to its counter,
// a finite nonzero value as three signed pieces to the bins hy_ens_split() names. Aggregated: as in hy_ens_cmm(), by the
// address of the first bin - the lanes of a wavefront which sample the same row at the same exponent are one group, and their
// pieces are summed, exactly, ahead of the three atomics.
__device__ __forceinline__ void hy_ens_sum(u64 *blk, const bool ok, const u64 v)
{
    const bool neg = (v >> 63) != 0u;
    const u64 mag = v & 0x7fffffffffffffffull;
    const bool inf = mag == 0x7ff0000000000000ull;
    if (ok && inf) atomicAdd(blk + HY_ENS_NBINS + (neg ? 1u : 0u), 1ull);
    unsigned p0, p1, p2;
    u64 *bins = blk + hy_ens_split(v, &p0, &p1, &p2);
    bool pend = ok && !inf && mag != 0u;
#if HY_ENS_AGG
    for (;;) {
        const u64 m = __builtin_amdgcn_ballot_w64(pend);
        if (m == 0u) break;
        const unsigned l = (unsigned)__builtin_ctzll(m);
        const bool same = pend && (u64)bins == hy_ens_rl64((u64)bins, l);
        u64 grp = __builtin_amdgcn_ballot_w64(same);
        const u64 ngrp = __builtin_amdgcn_ballot_w64(same && neg);
        u64 s0 = 0u, s1 = 0u, s2 = 0u;
        while (grp != 0u) {
            const unsigned j = (unsigned)__builtin_ctzll(grp);
            grp &= grp - 1u;
            const u64 a0 = (unsigned)__builtin_amdgcn_readlane((int)p0, (int)j);
            const u64 a1 = (unsigned)__builtin_amdgcn_readlane((int)p1, (int)j);
            const u64 a2 = (unsigned)__builtin_amdgcn_readlane((int)p2, (int)j);
            if (((ngrp >> j) & 1u) != 0u) {
                s0 -= a0; s1 -= a1; s2 -= a2;
            } else {
                s0 += a0; s1 += a1; s2 += a2;
            }
        }
        if ((threadIdx.x & 63u) == l) {
            if (s0 != 0u) atomicAdd(bins, s0);
            if (s1 != 0u) atomicAdd(bins + 1, s1);
            if (s2 != 0u) atomicAdd(bins + 2, s2);
        }
        pend = pend && !same;
    }
#else
    if (pend) {
        if (p0 != 0u) atomicAdd(bins, neg ? 0ull - p0 : (u64)p0);
        if (p1 != 0u) atomicAdd(bins + 1, neg ? 0ull - p1 : (u64)p1);
        if (p2 != 0u) atomicAdd(bins + 2, neg ? 0ull - p2 : (u64)p2);
    }
#endif
}
)HIP";
    }
    src << "\n// One value of an observable into its record. A NaN is skipped.\n"
           "__device__ __forceinline__ void hy_ens_merge(u64 *rec, const double y)\n{\n    const bool ok = y == y;\n"
           "    const u64 bits = (u64)__double_as_longlong(y);\n";
    if (l.count >= 0 || l.min >= 0 || l.max >= 0) {
        src << "    hy_ens_cmm(rec, ok, hy_ens_key(bits));\n";
    }
    if (l.sum >= 0) {
        src << "    hy_ens_sum(rec + " << l.sum << "u, ok, bits);\n";
    }
    if (l.sum_sq >= 0) {
        src << "    hy_ens_sum(rec + " << l.sum_sq << "u, ok, (u64)__double_as_longlong(__dmul_rn(y, y)));\n";
    }
    src << "}\n";
    return src.str();
}

} // namespace heyoka_amd::detail
