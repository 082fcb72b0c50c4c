// Ensemble histograms: the host side of the records and the device text of the bin search and the merge.
#include "grid_histogram.hpp"

#include <cmath>
#include <cstdlib>
#include <sstream>
#include <stdexcept>

namespace heyoka_amd::detail
{

hist_mode hist_mode_from_env()
{
    if (const char *env = std::getenv("HEYOKA_AMD_GRID_HIST")) {
        const std::string mode(env);
        for (int m = 0; m < 3; ++m) {
            if (mode == hist_mode_names[m]) {
                return static_cast<hist_mode>(m);
            }
        }
        if (!mode.empty()) {
            throw std::invalid_argument("Invalid value '" + mode + "' of HEYOKA_AMD_GRID_HIST: 'peratomic', 'aggregate' or 'hybrid'");
        }
    }
    return hist_default_mode;
}

unsigned hist_turns_from_env()
{
    if (const char *env = std::getenv("HEYOKA_AMD_GRID_HIST_TURNS")) {
        const std::string k(env);
        if (k == "1" || k == "2" || k == "4") {
            return static_cast<unsigned>(k[0] - '0');
        }
        if (!k.empty()) {
            throw std::invalid_argument("Invalid value '" + k + "' of HEYOKA_AMD_GRID_HIST_TURNS: '1', '2' or '4'");
        }
    }
    return hist_hybrid_turns;
}

namespace
{

void check_counts(const std::size_t *n_edges, std::size_t n_lists, std::size_t n_obs)
{
    if (n_lists != n_obs) {
        throw std::invalid_argument("The ensemble histograms of propagate_grid() need one list of bin edges per observable: "
                                    + std::to_string(n_obs) + " observable(s), " + std::to_string(n_lists) + " list(s)");
    }
    bool any = false;
    for (std::size_t o = 0; o < n_obs; ++o) {
        any = any || n_edges[o] != 0u;
    }
    if (!any) {
        throw std::invalid_argument("The ensemble histograms of propagate_grid() have no bin edges for any observable");
    }
    for (std::size_t o = 0; o < n_obs; ++o) {
        if (n_edges[o] == 1u) {
            throw std::invalid_argument("The bin edges of observable " + std::to_string(o)
                                        + " of propagate_grid() must be at least 2 finite, strictly increasing values");
        }
        if (n_edges[o] > hist_max_bins + 1u) {
            throw std::invalid_argument("The bin edges of observable " + std::to_string(o) + " of propagate_grid() make "
                                        + std::to_string(n_edges[o] - 1u) + " bins: at most " + std::to_string(hist_max_bins));
        }
    }
}

std::vector<std::size_t> counts_of(const std::vector<std::vector<double>> &edges)
{
    std::vector<std::size_t> n;
    for (const auto &e : edges) {
        n.push_back(e.size());
    }
    return n;
}

// The largest power of two which is not above n (n >= 1): the first stride of the bin search.
std::uint32_t first_stride(std::uint32_t n)
{
    std::uint32_t p = 1;
    while (2u * p <= n) {
        p *= 2u;
    }
    return p;
}

} // namespace

void check_ensemble_histograms(const std::vector<std::vector<double>> &edges, std::size_t n_obs)
{
    const auto n = counts_of(edges);
    check_counts(n.data(), n.size(), n_obs);
    for (std::size_t o = 0; o < edges.size(); ++o) {
        const auto &e = edges[o];
        for (std::size_t j = 0; j < e.size(); ++j) {
            if (!std::isfinite(e[j]) || (j != 0u && !(e[j - 1u] < e[j]))) {
                throw std::invalid_argument("The bin edges of observable " + std::to_string(o)
                                            + " of propagate_grid() must be at least 2 finite, strictly increasing values");
            }
        }
    }
}

hist_layout hist_layout_of(const std::size_t *n_edges, std::size_t n_obs)
{
    check_counts(n_edges, n_obs, n_obs);
    hist_layout l;
    for (std::size_t o = 0; o < n_obs; ++o) {
        const auto n = static_cast<std::uint32_t>(n_edges[o]);
        l.bins.push_back(n != 0u ? n - 1u : 0u);
        l.off.push_back(l.words);
        l.edge_off.push_back(l.n_edges);
        l.words += n != 0u ? n + 1u : 0u;
        l.n_edges += n;
    }
    return l;
}

hist_layout hist_layout_of(const std::vector<std::vector<double>> &edges)
{
    const auto n = counts_of(edges);
    return hist_layout_of(n.data(), n.size());
}

std::vector<double> hist_edge_table(const std::vector<std::vector<double>> &edges)
{
    std::vector<double> ret;
    for (const auto &e : edges) {
        ret.insert(ret.end(), e.begin(), e.end());
    }
    return ret;
}

std::vector<std::uint64_t> hist_init(const hist_layout &l, std::size_t n_grid)
{
    return std::vector<std::uint64_t>(n_grid * l.words, 0u);
}

std::uint32_t hist_slot(const double *e, std::uint32_t n_edges, double y)
{
    std::uint32_t s = 0;
    for (auto p = first_stride(n_edges); p != 0u; p >>= 1) {
        const auto t = s + p;
        const auto j = (t <= n_edges ? t : n_edges) - 1u;
        const bool up = t <= n_edges && e[j] <= y;
        s = up ? t : s;
    }
    return s;
}

void hist_add(const hist_layout &l, const double *table, std::uint64_t *rec, std::size_t o, double y)
{
    if (y != y || l.bins[o] == 0u) {
        return;
    }
    rec[l.off[o] + hist_slot(table + l.edge_off[o], l.bins[o] + 1u, y)] += 1u;
}

void hist_merge(const hist_layout &l, std::uint64_t *dst, const std::uint64_t *src, std::size_t n_grid)
{
    for (std::size_t w = 0; w < n_grid * l.words; ++w) {
        dst[w] += src[w];
    }
}

std::int64_t hist_rank_slot(const hist_layout &l, const std::uint64_t *rec, std::size_t o, std::uint64_t k)
{
    if (k == 0u || l.bins[o] == 0u) {
        return -1;
    }
    std::uint64_t cum = 0;
    for (std::uint32_t s = 0; s < l.bins[o] + 2u; ++s) {
        cum += rec[l.off[o] + s];
        if (cum >= k) {
            return static_cast<std::int64_t>(s);
        }
    }
    return -1;
}

std::string hist_device_text(const hist_layout &l, hist_mode mode, unsigned turns, bool with_ens)
{
    std::ostringstream src;
    src << "\n// Ensemble histograms (DESIGN 4.3h): HY_HIST_W 64-bit counters per grid point, the records of the observables with edges\n"
           "// in slot order; behind the records of all grid points their shadow copy, then the edge tables. Integer atomics only.\n"
           "#define HY_HIST_W "
        << l.words << "u\n#define HY_HIST_MODE " << static_cast<int>(mode) << "\n#define HY_HIST_TURNS " << turns
        << "u\n// The words of the ensemble statistics per grid point, which stand ahead of the histograms.\n#define HY_HIST_ENSW "
        << (with_ens ? "(HY_NOUT * HY_ENS_WORDS)" : "0u") << R"HIP(

// The records of grid point g, and the edge tables, behind the start outp of the output of a call over n_grid points. Per
// lane and in VGPRs (the empty asm statements), like the other addresses of the sampling: as uniform values they would hold
// pairs of SGPRs next to the masks of the merge loops, and the wave has 102.
__device__ __forceinline__ u64 *hy_hist_rec(double *outp, const unsigned n_grid, const unsigned g)
{
    u64 *rec = (u64 *)outp;
    unsigned ng = n_grid;
    asm volatile("" : "+v"(rec), "+v"(ng));
    return rec + (u64)ng * HY_HIST_ENSW + (u64)g * HY_HIST_W;
}
__device__ __forceinline__ const double *hy_hist_edges(double *outp, const unsigned n_grid)
{
    const double *e = (const double *)outp;
    unsigned ng = n_grid;
    asm volatile("" : "+v"(e), "+v"(ng));
    return e + 2u * (u64)ng * (HY_HIST_ENSW + HY_HIST_W);
}

// The slot of y among the n edges e, #{ j : e[j] <= y }: a search by halving strides from p, the largest power of two not above
// n - the same number of steps in every lane, comparisons only, every load inside the table. A NaN gives slot 0.
__device__ __forceinline__ unsigned hy_hist_slot(const double *e, const unsigned n, const unsigned p0, const double y)
{
    unsigned s = 0u;
#pragma unroll
    for (unsigned p = p0; p != 0u; p >>= 1) {
        const unsigned t = s + p;
        const unsigned j = (t <= n ? t : n) - 1u;
        const bool up = t <= n && e[j] <= y;
        s = up ? t : s;
    }
    return s;
}

// The 64-bit value v of lane l (uniform, a lane which is active here).
__device__ __forceinline__ u64 hy_hist_rl64(const u64 v, const unsigned l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)l);
    return ((u64)hi << 32) | lo;
}

// One count into the word of every lane with pend set. Aggregated (HY_HIST_MODE 1): the lanes whose word is the one of the first
// pending lane are counted in that lane, which issues the atomic; then the next group, until no lane is left. Hybrid (2): at
// most HY_HIST_TURNS such turns, then the lanes still pending issue their own. Every lane which arrives here takes every turn
// (the ballots are uniform); only the lanes of a ballot mask are read.
__device__ __forceinline__ void hy_hist_count(u64 *word, bool pend)
{
#if HY_HIST_MODE == 0
    if (pend) atomicAdd(word, 1ull);
#else
#if HY_HIST_MODE == 2
#pragma unroll
    for (unsigned turn = 0; turn < HY_HIST_TURNS; ++turn) {
#else
    for (;;) {
#endif
        const u64 m = __builtin_amdgcn_ballot_w64(pend);
        if (m == 0u) break;
        const unsigned l = (unsigned)__builtin_ctzll(m);
        const bool same = pend && (u64)word == hy_hist_rl64((u64)word, l);
        const u64 grp = __builtin_amdgcn_ballot_w64(same);
        if ((threadIdx.x & 63u) == l) atomicAdd(word, (u64)__builtin_popcountll(grp));
        pend = pend && !same;
    }
#if HY_HIST_MODE == 2
    if (pend) atomicAdd(word, 1ull);
#endif
#endif
}
)HIP";
    return src.str();
}

// The call of the search and the merge for observable o of the layout, on the value named y at grid point g.
std::string hist_device_call(const hist_layout &l, std::size_t o, const std::string &y)
{
    const auto n = l.bins[o] + 1u;
    std::ostringstream src;
    src << "hy_hist_count(hy_hist_rec(outp, a.n_grid, g) + (" << l.off[o] << "u + hy_hist_slot(hy_hist_edges(outp, a.n_grid) + "
        << l.edge_off[o] << "u, " << n << "u, " << first_stride(n) << "u, " << y << ")), " << y << " == " << y << ");\n";
    return src.str();
}

} // namespace heyoka_amd::detail
