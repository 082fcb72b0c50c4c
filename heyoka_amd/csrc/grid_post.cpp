// Post-step kernels of the device-driven sweep loops of propagate_until() and propagate_grid() (tab_propagate.cpp).
#include "tab_impl.hpp"

#include <set>

#include "cfunc.hpp"
#include "grid_observables.hpp"

namespace heyoka_amd::detail
{

grid_sampling::grid_sampling(std::optional<std::vector<expression>> obs, std::optional<std::vector<grid_statistic>> stats,
                             std::optional<std::vector<ensemble_statistic>> ens,
                             std::optional<std::vector<std::vector<double>>> hist)
    : observables(std::move(obs)), statistics(std::move(stats)), ensemble(std::move(ens)), histograms(std::move(hist))
{
    if (histograms) {
        if (!observables) {
            throw std::invalid_argument(ensemble_histograms_need_observables);
        }
        if (statistics) {
            throw std::invalid_argument(ensemble_histograms_exclude_statistics);
        }
        check_ensemble_histograms(*histograms, observables->size());
    }
    if (ensemble) {
        if (!observables) {
            throw std::invalid_argument(ensemble_statistics_need_observables);
        }
        if (statistics) {
            throw std::invalid_argument(ensemble_statistics_exclude_statistics);
        }
        check_ensemble_statistics(*ensemble);
    }
    if (statistics) {
        if (!observables) {
            throw std::invalid_argument(grid_statistics_need_observables);
        }
        check_grid_statistics(*statistics);
    }
}

std::string grid_obs_key(const grid_sampling &gs)
{
    std::string key;
    for (const auto &ex : gs.observables.value()) {
        key += ex.to_string() + ";";
    }
    const char *env = std::getenv("HEYOKA_AMD_GRID_OBS");
    key += std::string("|") + (env != nullptr ? env : "");
    if (gs.statistics) {
        key += "|statistics:";
        for (const auto s : *gs.statistics) {
            key += std::to_string(static_cast<int>(s)) + ",";
        }
    }
    if (gs.ensemble) {
        key += "|ensemble:";
        for (const auto s : *gs.ensemble) {
            key += std::to_string(static_cast<int>(s)) + ",";
        }
        const char *ens_env = std::getenv("HEYOKA_AMD_GRID_ENS");
        key += std::string("|") + (ens_env != nullptr ? ens_env : "");
    }
    if (gs.histograms) {
        key += "|histograms:";
        for (const auto &e : *gs.histograms) {
            key += std::to_string(e.size()) + ",";
        }
        const char *hist_env = std::getenv("HEYOKA_AMD_GRID_HIST");
        key += std::string("|") + (hist_env != nullptr ? hist_env : "");
        const char *turns_env = std::getenv("HEYOKA_AMD_GRID_HIST_TURNS");
        key += std::string("|") + (turns_env != nullptr ? turns_env : "");
    }
    return key;
}

// ---- grid statistics ----
void check_grid_statistics(const std::vector<grid_statistic> &stats)
{
    if (stats.empty()) {
        throw std::invalid_argument("The list of statistics of propagate_grid() is empty");
    }
    std::set<int> seen;
    for (const auto s : stats) {
        const auto code = static_cast<int>(s);
        if (code < 0 || code >= n_grid_statistics) {
            throw std::invalid_argument("The statistic code " + std::to_string(code) + " of propagate_grid() is unknown");
        }
        if (!seen.insert(code).second) {
            throw std::invalid_argument(std::string("The statistic '") + grid_statistic_names[code]
                                        + "' of propagate_grid() is named twice");
        }
    }
}

std::vector<grid_statistic> grid_statistics_from_codes(const int *codes, std::size_t n)
{
    std::vector<grid_statistic> ret;
    for (std::size_t k = 0; k < n; ++k) {
        ret.push_back(static_cast<grid_statistic>(codes[k]));
    }
    check_grid_statistics(ret);
    return ret;
}

namespace
{

// The slots of the accumulators of one observable, by statistic (-1: not kept): those of the output, o * n_stat + position in
// the list, and behind all of them the extremum a t_min / t_max needs when it was asked for alone.
struct stat_slots {
    int slot[n_grid_statistics];
};

std::vector<stat_slots> grid_stat_slots(std::uint32_t n_obs, const std::vector<grid_statistic> &stats, std::uint32_t &n_slots)
{
    const auto n_stat = static_cast<std::uint32_t>(stats.size());
    n_slots = n_obs * n_stat;
    std::vector<stat_slots> ret(n_obs);
    for (std::uint32_t o = 0; o < n_obs; ++o) {
        auto &s = ret[o].slot;
        std::fill(std::begin(s), std::end(s), -1);
        for (std::uint32_t k = 0; k < n_stat; ++k) {
            s[static_cast<int>(stats[k])] = static_cast<int>(o * n_stat + k);
        }
        for (const auto &[tm, m] : {std::pair{grid_statistic::t_min, grid_statistic::min}, std::pair{grid_statistic::t_max, grid_statistic::max}}) {
            if (s[static_cast<int>(tm)] >= 0 && s[static_cast<int>(m)] < 0) {
                s[static_cast<int>(m)] = static_cast<int>(n_slots++);
            }
        }
    }
    return ret;
}

} // namespace

grid_obs_section make_grid_obs_section(const grid_sampling &gs, const std::vector<expression> &state_vars, std::uint32_t n_par)
{
    const auto &obs = gs.observables.value();
    if (obs.empty()) {
        throw std::invalid_argument("The list of observables of propagate_grid() is empty");
    }
    const section_wording w{
        [](std::size_t o, const std::string &v) {
            return "The observable " + std::to_string(o) + " of propagate_grid() uses the variable '" + v
                   + "', which is not a state variable of the system";
        },
        [](std::uint32_t i, std::uint32_t n) {
            return "An observable of propagate_grid() uses par[" + std::to_string(i) + "], but the integrator has "
                   + std::to_string(n) + " parameter(s)";
        }};
    grid_obs_section ret;
    static_cast<expr_section &>(ret) = make_expr_section(obs, state_vars, n_par, w);
    ret.n_obs = static_cast<std::uint32_t>(obs.size());
    ret.staged = ret.reads.size() > grid_obs_max_register_rows;
    if (const char *env = std::getenv("HEYOKA_AMD_GRID_OBS")) {
        const std::string mode(env);
        if (mode == "registers") {
            ret.staged = false;
        } else if (mode == "staged") {
            ret.staged = true;
        } else if (!mode.empty()) {
            throw std::invalid_argument("Invalid value '" + mode + "' of HEYOKA_AMD_GRID_OBS: 'registers' or 'staged'");
        }
    }
    if (gs.statistics) {
        ret.stats = *gs.statistics;
        (void)grid_stat_slots(ret.n_obs, ret.stats, ret.n_slots);
    }
    if (gs.ensemble) {
        ret.ens = *gs.ensemble;
        ret.ens_rec = ens_layout_of(ret.ens);
        if (const char *env = std::getenv("HEYOKA_AMD_GRID_ENS")) {
            const std::string mode(env);
            if (mode == "peratomic") {
                ret.ens_aggregate = false;
            } else if (!mode.empty() && mode != "aggregate") {
                throw std::invalid_argument("Invalid value '" + mode + "' of HEYOKA_AMD_GRID_ENS: 'aggregate' or 'peratomic'");
            }
        }
    }
    if (gs.histograms) {
        ret.hist = hist_layout_of(*gs.histograms);
        ret.hist_merge_mode = hist_mode_from_env();
        ret.hist_turns = hist_turns_from_env();
    }
    return ret;
}

namespace
{

// The observable section of the module: the dense output of one state row (the loop of the plain hy_grid_post, operation by
// operation) and hy_obs_section(), the straight-line code of emit_order0() with its stores. Registers: the samples arrive as
// arguments x<row>; staged: they are read from a.stage at the point of use, through a volatile pointer - the loads are not
// replaced by the values just stored, which would keep every sample alive in a register after all.
std::string grid_obs_device_functions(const grid_obs_section &sec)
{
    const auto &p = sec.prog;
    // The numerical constants of the section which are not inline constants of the instruction set - a pair of SGPRs each,
    // and the compiler moves all of them ahead of the grid loop (44 SGPRs for the energy of the outer Solar System, more
    // than are left) - become named values c<k> in VGPRs: the same bits in the same operations.
    std::map<const operand *, std::string> lit_names;
    std::vector<std::string> lit_decls;
    {
        std::map<std::uint64_t, std::string> by_bits;
        const auto visit = [&](const operand &o) {
            if (o.type != operand::kind::num) {
                return;
            }
            const auto av = std::abs(o.value);
            if (av == 0. || av == 0.5 || av == 1. || av == 2. || av == 4.) {
                return;
            }
            std::uint64_t bits = 0;
            std::memcpy(&bits, &o.value, sizeof(bits));
            auto it = by_bits.find(bits);
            if (it == by_bits.end()) {
                it = by_bits.emplace(bits, "c" + std::to_string(by_bits.size())).first;
                lit_decls.push_back("double " + it->second + " = " + fp_literal(o.value) + ";\nasm volatile(\"\" : \"+v\"("
                                    + it->second + "));\n");
            }
            lit_names.emplace(&o, it->second);
        };
        for (const auto &n : p.nodes) {
            for (const auto &o : n.args) {
                visit(o);
            }
        }
        for (const auto &d : p.sv_defs) {
            visit(d);
        }
    }
    const auto code = emit_order0(
        p,
        [&](std::uint32_t r) {
            return sec.staged ? "((const volatile double *)stg)[(u64)" + std::to_string(r) + "u * N]" : "x" + std::to_string(r);
        },
        &lit_names);
    std::ostringstream src;
    src << "\n// The state rows the observables read.\n#define HY_NROWS " << sec.reads.size() << "u\n__device__ const unsigned hy_obs_rows["
        << (sec.reads.empty() ? "1" : "HY_NROWS") << "] = {";
    for (std::size_t j = 0; j < sec.reads.size(); ++j) {
        src << (j != 0u ? ", " : "") << sec.reads[j] << "u";
    }
    // (Observables of the parameters and the time alone read no row: no array of length zero.)
    src << (sec.reads.empty() ? "0u" : "") << "};\n";
    const bool folds = !sec.stats.empty();
    const bool ens = !sec.ens.empty();
    const bool hist = sec.hist.words != 0u;
    if (hist) {
        // (Behind the text of the ensemble statistics, if any, whose HY_ENS_WORDS places the histogram records.)
        src << (ens ? ens_device_text(sec.ens_rec, sec.ens_aggregate) : std::string{})
            << hist_device_text(sec.hist, sec.hist_merge_mode, sec.hist_turns, ens) << R"HIP(
// The observables of lane i at grid point g and time t_hi, merged into the records behind outp, the start of the output: those
// of the ensemble statistics, if any, and the counters of the histograms (stg points to the staged samples of the lane).
__device__ __forceinline__ void hy_obs_section(const hy_grid_args &a, const u64 i, const u64 N, double *outp, const unsigned g, const double t_hi
)HIP";
    } else if (ens) {
        src << ens_device_text(sec.ens_rec, sec.ens_aggregate) << R"HIP(
// The observables of lane i at grid point g and time t_hi, merged into the records (g * HY_NOUT + o) behind outp, the start of
// the output (stg points to the staged samples of the lane).
__device__ __forceinline__ void hy_obs_section(const hy_grid_args &a, const u64 i, const u64 N, double *outp, const unsigned g, const double t_hi
)HIP";
    } else if (folds) {
        src << R"HIP(
// Grid statistics: the accumulators of a lane are the slots out[s * N + i], s < HY_NSLOT - those of the output first -, and
// out[(HY_NSLOT + s) * N + i] is their shadow copy.
#define HY_NSLOT )HIP" << sec.n_slots << R"HIP(u

// The observables of lane i at grid point g and time t_hi, folded into the accumulators of the lane: outp points to out[i]
// (and stg to the staged samples of the lane). g == 0: the accumulators start from these values.
__device__ __forceinline__ void hy_obs_section(const hy_grid_args &a, const u64 i, const u64 N, double *outp, const unsigned g, const double t_hi
)HIP";
    } else {
        src << R"HIP(
// The observables of lane i at grid point g and time t_hi, stored to out[(g * HY_NOUT + o) * N + i]: outp points to out[i]
// (and stg to the staged samples of the lane).
__device__ __forceinline__ void hy_obs_section(const hy_grid_args &a, const u64 i, const u64 N, double *outp, const unsigned g, const double t_hi
)HIP";
    }
    if (sec.staged) {
        src << ", const double *stg";
    } else {
        for (const auto r : sec.reads) {
            src << ", const double x" << r;
        }
    }
    src << ")\n{\n";
    for (std::uint32_t k = 0; k < p.n_par; ++k) {
        src << "const double par_" << k << " = a.pars[(u64)" << k << "u * N + i];\n";
    }
    if (!p.time_dependent) {
        src << "(void)t_hi;\n";
    }
    for (const auto &d : lit_decls) {
        src << d;
    }
    src << code.body;
    if (hist) {
        // The merges, behind the last value of the section, on the same opaque values: the records of the ensemble statistics
        // first, with the text of their own variant, then the bin search and the count of every observable with edges.
        for (std::size_t o = 0; o < code.outs.size(); ++o) {
            src << "double y" << o << " = " << code.outs[o] << ";\nasm volatile(\"\" : \"+v\"(y" << o << "));\n";
        }
        for (std::size_t o = 0; ens && o < code.outs.size(); ++o) {
            src << "hy_ens_merge((u64 *)outp + ((u64)g * HY_NOUT + " << o << "u) * HY_ENS_WORDS, y" << o << ");\n";
        }
        for (std::size_t o = 0; o < code.outs.size(); ++o) {
            if (sec.hist.bins[o] != 0u) {
                src << hist_device_call(sec.hist, o, "y" + std::to_string(o));
            }
        }
        src << "}\n";
        return src.str();
    }
    if (ens) {
        // The merge, behind the last value of the section, as with the grid statistics: the values are opaque to the backend.
        for (std::size_t o = 0; o < code.outs.size(); ++o) {
            src << "double y" << o << " = " << code.outs[o] << ";\nasm volatile(\"\" : \"+v\"(y" << o << "));\n";
        }
        for (std::size_t o = 0; o < code.outs.size(); ++o) {
            src << "hy_ens_merge((u64 *)outp + ((u64)g * HY_NOUT + " << o << "u) * HY_ENS_WORDS, y" << o << ");\n";
        }
        src << "}\n";
        return src.str();
    }
    if (!folds) {
        for (std::size_t o = 0; o < code.outs.size(); ++o) {
            src << "outp[((u64)g * HY_NOUT + " << o << "u) * N] = " << code.outs[o] << ";\n";
        }
        src << "}\n";
        return src.str();
    }
    // The merge, behind the last value of the section: its temporaries are dead, the accumulators come from memory and go
    // back there - nothing is held in a register across the grid loop. A value which went through an asm operand is opaque
    // to the backend: the addition of `sum` is not contracted with a product which ends the observable.
    std::uint32_t n_slots = 0;
    const auto slots = grid_stat_slots(sec.n_obs, sec.stats, n_slots);
    const auto acc = [](int s) { return "outp[(u64)" + std::to_string(s) + "u * N]"; };
    const auto sl = [&](std::size_t o, grid_statistic s) { return slots[o].slot[static_cast<int>(s)]; };
    for (std::size_t o = 0; o < code.outs.size(); ++o) {
        src << "double y" << o << " = " << code.outs[o] << ";\nasm volatile(\"\" : \"+v\"(y" << o << "));\n";
    }
    src << "if (g == 0u) {\n";
    for (std::size_t o = 0; o < code.outs.size(); ++o) {
        for (const auto s : {grid_statistic::min, grid_statistic::max, grid_statistic::sum, grid_statistic::last}) {
            if (sl(o, s) >= 0) {
                src << acc(sl(o, s)) << " = y" << o << ";\n";
            }
        }
        for (const auto s : {grid_statistic::t_min, grid_statistic::t_max}) {
            if (sl(o, s) >= 0) {
                src << acc(sl(o, s)) << " = t_hi;\n";
            }
        }
        if (sl(o, grid_statistic::count) >= 0) {
            src << acc(sl(o, grid_statistic::count)) << " = 1.0;\n";
        }
    }
    src << "} else {\n";
    for (std::size_t o = 0; o < code.outs.size(); ++o) {
        const auto extremum = [&](grid_statistic m, grid_statistic tm, const char *cmp) {
            if (sl(o, m) < 0) {
                return;
            }
            src << "{ const double m = " << acc(sl(o, m)) << "; if (y" << o << " " << cmp << " m || m != m) { " << acc(sl(o, m))
                << " = y" << o << "; ";
            if (sl(o, tm) >= 0) {
                src << acc(sl(o, tm)) << " = t_hi; ";
            }
            src << "} }\n";
        };
        extremum(grid_statistic::min, grid_statistic::t_min, "<");
        extremum(grid_statistic::max, grid_statistic::t_max, ">");
        if (sl(o, grid_statistic::sum) >= 0) {
            src << acc(sl(o, grid_statistic::sum)) << " = __dadd_rn(" << acc(sl(o, grid_statistic::sum)) << ", y" << o << ");\n";
        }
        if (sl(o, grid_statistic::last) >= 0) {
            src << acc(sl(o, grid_statistic::last)) << " = y" << o << ";\n";
        }
        if (sl(o, grid_statistic::count) >= 0) {
            src << acc(sl(o, grid_statistic::count)) << " = " << acc(sl(o, grid_statistic::count)) << " + 1.0;\n";
        }
    }
    src << "}\n}\n";
    return src.str();
}

// The call of hy_obs_section() behind the samples x<row> / the staged samples.
std::string grid_obs_call(const grid_obs_section &sec, const char *outp, const char *stg, const char *xs, const char *g, const char *t)
{
    std::string ret = std::string("hy_obs_section(a, i, N, ") + outp + ", " + g + ", " + t;
    if (sec.staged) {
        ret += std::string(", ") + stg;
    } else {
        for (std::size_t j = 0; j < sec.reads.size(); ++j) {
            ret += ", " + std::string(xs) + "[" + std::to_string(j) + "]";
        }
    }
    return ret + ");\n";
}

} // namespace

// The dense output of one state row inside hy_grid_post - c points to its order-0 coefficient, hd is the time from the start
// of the step, the sample is res -: shared, text for text, by the plain kernel and by the kernel with an observable section.
constexpr const char *dense_row_text = R"HIP(#if HY_HA
            double res = c[0], comp = 0.0, cur_h = hd;
            for (unsigned k = 1; k <= HY_ORDER; ++k) {
                const double tmp = c[(u64)k * N] * cur_h;
                const double y = tmp - comp;
                const double t = res + y;
                comp = (t - res) - y;
                res = t;
                cur_h = cur_h * hd;
            }
#else
            double res = c[(u64)HY_ORDER * N];
            for (unsigned k = 1; k <= HY_ORDER; ++k) {
                res = c[(u64)(HY_ORDER - k) * N] + res * hd;
            }
#endif
)HIP";

// Post-step kernel of the device-resident propagate_grid() loop: the per-lane body of the reference's loop
// (src/taylor_adaptive_batch.cpp:1760-2040) - step counters, remaining time, dense output at every grid
// point inside the step just taken (h' = t_grid - (t_now - last_h) in double-length arithmetic, Horner or
// compensated summation as in taylor_add_d_out_function()), limit of the next step.
std::string make_grid_source(std::uint32_t order, std::uint32_t dim, bool ha)
{
    return make_grid_source(order, dim, ha, nullptr);
}

std::string make_grid_source(std::uint32_t order, std::uint32_t dim, bool ha, const grid_obs_section *sec)
{
    std::ostringstream src;
    src << emit_detail::prelude();
    if (sec != nullptr) {
        src << emit_detail::rules_source(sec->prog);
    }
    src << "#define HY_ORDER " << order << "u\n#define HY_DIM " << dim << "u\n#define HY_HA " << (ha ? 1 : 0) << "\n";
    if (sec != nullptr) {
        src << "#define HY_NOUT " << sec->n_obs << "u\n";
    }
    const char *const ncol = sec != nullptr ? "HY_NOUT" : "HY_DIM";
    src << "\n" << grid_kargs_text() << R"HIP(
// Post-step kernel of the device-driven propagate_until() lock-step loop (callbacks / continuous output): the
// per-lane bookkeeping of src/taylor_adaptive_batch.cpp:1395-1440 (step counters, min/max |h|, remaining time, limit of
// the next step). counters[0] = lanes done in this sweep, counters[1] = lanes with a non-finite state. The final
// times are in the (double-length) grid row 0: grid[i] = hi, out[i] = lo.
// One atomic per wavefront instead of one per lane: the lanes which reach a call site with pred set elect the lowest of
// them, which adds their number. (hy_grid_post counts the lanes which are NOT through their grid - every lane of every
// sweep: 262 144 atomics on one address were 6 ms of a 6.5-ms sweep, profiles/r05_grid_sweeps.log.)
__device__ __forceinline__ void hy_count(unsigned *p, bool pred)
{
    const u64 m = __builtin_amdgcn_ballot_w64(pred);
    if (pred && (unsigned)__builtin_ctzll(m) == (threadIdx.x & 63u)) atomicAdd(p, (unsigned)__builtin_popcountll(m));
}

// Independent semantics (hy_grid_args::retired != nullptr; the branches below do not run otherwise). A system is retired by
// the step which ends in a stopping terminal event (outcome -index - 1) or in a non-finite state: the outcome becomes sticky
// in retired[i] (0: not retired) and the limit of its next steps is zero, so that it takes zero-length steps like a system
// which has reached its final time - state, time, cooldowns, step count and min / max |h| stay those of that step. The
// zero-length steps report time_limit: the sticky outcome is put back after each of them. counters[4] / [5]: systems
// retired by events / as non-finite so far.
// Returns true for a system retired in an EARLIER sweep: nothing else is to be done for it.
__device__ __forceinline__ bool hy_indep_retired(const hy_grid_args &a, u64 i)
{
    const i64 so = a.retired[i];
    if (so == 0) return false;
    a.outcome_w[i] = so;
    a.lim[i] = 0.0;
    // (Frozen cooldowns: a zero-length step ages a cooldown by nothing, but it ends one of duration zero - the one the
    // retiring event may have set.)
    // (so > HY_OC_SUCCESS: a stopping terminal event. A system retired by a step_action carries cb_stop: no event, no cooldown,
    // and it is counted by the action's own counter.)
    if (so > HY_OC_SUCCESS && a.cd_active != nullptr) {
        const u64 p = (u64)(-so - 1) * a.N + i;
        if (a.cd_second[p] == 0.0) a.cd_active[p] = 1;
    }
    hy_count(a.counters + 4, so > HY_OC_SUCCESS);
    hy_count(a.counters + 5, so == HY_OC_ERR_NF_STATE);
    return true;
}

extern "C" __global__ void __launch_bounds__(256) hy_until_post(const hy_grid_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (i >= N) return;
    const bool indep = a.retired != nullptr;
    if (indep && hy_indep_retired(a, i)) {
        hy_count(a.counters, true);
        return;
    }
    const i64 oc = a.outcome[i];
    const double h = a.last_h[i];
    if (oc == HY_OC_ERR_NF_STATE) {
        if (indep) {
            // (Retired as non-finite: done as far as the loop is concerned, the other systems carry on.)
            a.retired[i] = oc;
            a.lim[i] = 0.0;
            hy_count(a.counters, true);
            hy_count(a.counters + 5, true);
            return;
        }
        hy_count(a.counters + 1, true);
        return;
    }
    a.n_steps[i] += (h != 0.0) ? 1u : 0u;
    if (oc == HY_OC_SUCCESS) {
        const double ah = fabs(h);
        a.min_h[i] = hy_min(a.min_h[i], ah);
        a.max_h[i] = hy_max(a.max_h[i], ah);
    }
    // Stopping terminal event: outcome -index - 1 (src/taylor_adaptive_batch.cpp:1411).
    const bool stopped = oc > HY_OC_SUCCESS && oc < 0;
    hy_count(a.counters + 2, stopped);
    hy_df rem; rem.hi = a.rem_hi[i]; rem.lo = a.rem_lo[i];
    // (Independent semantics: the system retired by this step counts as done; the bookkeeping of the step is the one above
    // and below - what the same step leaves behind when it ends the loop of the whole batch.)
    const bool retire = indep && stopped;
    if (retire) {
        a.retired[i] = oc;
        hy_count(a.counters + 4, true);
    }
    hy_count(a.counters, h == rem.hi || retire);
    if (h == rem.hi) {
        rem.hi = 0.0; rem.lo = 0.0;
    } else {
        hy_df tcur; tcur.hi = a.thi[i]; tcur.lo = a.tlo[i];
        hy_df tf; tf.hi = a.grid[i]; tf.lo = a.out[i];
        rem = hy_df_sub(tf, tcur);
    }
    a.rem_hi[i] = rem.hi; a.rem_lo[i] = rem.lo;
    hy_df m; m.lo = 0.0;
    double lim;
    if (a.t_dir[i] != 0) { m.hi = a.mdt[i]; lim = hy_df_lt(rem, m) ? rem.hi : m.hi; }
    else { m.hi = -a.mdt[i]; lim = hy_df_lt(m, rem) ? rem.hi : m.hi; }
    a.lim[i] = retire ? 0.0 : lim;
}

// Independent semantics, events applied on the device: behind hy_ev_native, which has given the first terminal event of a
// system its cooldown and the continuing outcome `index` - a terminal event WITHOUT a callback stops (te_stop[index] != 0:
// the flag is data), outcome -index - 1.
)HIP" << ev_stop_kargs_text() << R"HIP(extern "C" __global__ void __launch_bounds__(256) hy_ev_stop(const hy_ev_stop_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.N) return;
    const i64 oc = a.outcome[i];
    if (oc >= 0 && oc < (i64)a.n_te && a.te_stop[oc] != 0) a.outcome[i] = -oc - 1;
}

// Independent semantics: the loop was ended by max_steps or by the step callback - the systems which are neither retired
// nor done (remaining time zero) report override_oc (step_limit / cb_stop), the others keep their outcomes.
extern "C" __global__ void __launch_bounds__(256) hy_indep_override(const hy_grid_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.N) return;
    if (a.retired[i] != 0) return;
    const bool done = (a.gidx != nullptr) ? (a.gidx[i] >= a.n_grid) : (a.rem_hi[i] == 0.0 && a.rem_lo[i] == 0.0);
    if (!done) a.outcome_w[i] = a.override_oc;
}
)HIP";
    if (sec != nullptr) {
        src << grid_obs_device_functions(*sec);
    }
    src << R"HIP(
extern "C" __global__ void __launch_bounds__(256) hy_grid_post(const hy_grid_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (i >= N) return;
    if (a.launch_nf != nullptr && *a.launch_nf != 0u) {
        if (i == 0u) a.counters[3] = 1u;
        return;
    }
    if (a.gidx_prev != nullptr) a.gidx_prev[i] = a.gidx[i];
    const bool indep = a.retired != nullptr;
    // (A retired system is through its grid: it is not counted in counters[0].)
    if (indep && hy_indep_retired(a, i)) return;
    const i64 oc = a.outcome[i];
    const double h = a.last_h[i];
    if (oc == HY_OC_ERR_NF_STATE) {
        // (A launch of several steps per lane - per-lane semantics: the steps before the non-finite one count.)
        if (a.acc_n_steps != nullptr) {
            a.acc_n_steps[i] += a.n_steps[i];
            a.acc_min_h[i] = hy_min(a.acc_min_h[i], a.min_h[i]);
            a.acc_max_h[i] = hy_max(a.acc_max_h[i], a.max_h[i]);
        }
        if (indep) {
            // (Retired as non-finite: no samples of this step, the remaining rows stay NaN, the other systems carry on.)
            a.retired[i] = oc;
            a.lim[i] = 0.0;
            a.gidx[i] = a.n_grid;
            if (a.next_tg != nullptr) a.next_tg[i] = (a.t_dir[i] != 0) ? __builtin_inf() : -__builtin_inf();
            hy_count(a.counters + 5, true);
            return;
        }
        hy_count(a.counters + 1, true);
        return;
    }
    if (a.acc_n_steps != nullptr) {
        // (A launch of several steps per lane: its own counters and extrema.)
        a.acc_n_steps[i] += a.n_steps[i];
        a.acc_min_h[i] = hy_min(a.acc_min_h[i], a.min_h[i]);
        a.acc_max_h[i] = hy_max(a.acc_max_h[i], a.max_h[i]);
    } else {
        a.n_steps[i] += (h != 0.0) ? 1u : 0u;
        if (oc == HY_OC_SUCCESS) {
            const double ah = fabs(h);
            a.min_h[i] = hy_min(a.min_h[i], ah);
            a.max_h[i] = hy_max(a.max_h[i], ah);
        }
    }
    // Stopping terminal event: outcome -index - 1 (:1903-1908).
    const bool stopped = oc > HY_OC_SUCCESS && oc < 0;
    hy_count(a.counters + 2, stopped);
    // (Independent semantics: the system is retired by this step. It takes the samples inside the truncated step below,
    // like the step which ends the loop of the whole batch; then its grid index goes to the end - not through the
    // done_lane branch, which would sample every remaining point.)
    const bool retire = indep && stopped;
    if (retire) {
        a.retired[i] = oc;
        hy_count(a.counters + 4, true);
    }
    hy_df tcur; tcur.hi = a.thi[i]; tcur.lo = a.tlo[i];
    hy_df rem; rem.hi = a.rem_hi[i]; rem.lo = a.rem_lo[i];
    const unsigned ng = a.n_grid;
    // (A launch of several steps per lane: the stored remaining time is the one before its FIRST step - the stepper says
    // whether its last step was the one clamped to the remaining time.)
    const bool clamped_to_rem = (a.grid_done != nullptr) ? (a.grid_done[i] != 0.0) : (h == rem.hi);
    if (clamped_to_rem) {
        rem.hi = 0.0; rem.lo = 0.0;
    } else {
        hy_df tl; tl.hi = a.grid[(u64)(ng - 1u) * N + i]; tl.lo = 0.0;
        rem = hy_df_sub(tl, tcur);
    }
    a.rem_hi[i] = rem.hi; a.rem_lo[i] = rem.lo;
    // Time interval covered by the step, and the start of the step for the dense output.
    hy_df hh; hh.hi = h; hh.lo = 0.0;
    const hy_df tstart = hy_df_sub(tcur, hh);
    const bool fwd = !hy_df_lt(tcur, tstart);
    const hy_df t0 = fwd ? tstart : tcur, t1 = fwd ? tcur : tstart;
    const bool done_lane = (rem.hi == 0.0 && rem.lo == 0.0);
)HIP";
    if (sec != nullptr) {
        // The addresses the sampling uses, per lane and in VGPRs (the empty asm statements): as uniform base addresses they
        // would hold a pair of SGPRs each across the whole loop, next to the literals of the section, which are moved ahead
        // of the loop as well - the wave has 102 SGPRs, and 512 VGPRs per lane at 256 lanes per workgroup.
        src << "    const double *tc0 = a.tc + i;\n    asm volatile(\"\" : \"+v\"(tc0));\n";
        if (!sec->merges()) {
            src << "    double *out0 = a.out + i;\n    asm volatile(\"\" : \"+v\"(out0));\n";
        }
        if (sec->staged) {
            src << "    double *stg = a.stage + i;\n    asm volatile(\"\" : \"+v\"(stg));\n";
        }
        if (!sec->stats.empty()) {
            src << "    bool shadowed = false;\n";
        }
    }
    src << R"HIP(    unsigned g = a.gidx[i];
    while (g < ng) {
        hy_df tg; tg.hi = a.grid[(u64)g * N + i]; tg.lo = 0.0;
        const bool avail = (!hy_df_lt(tg, t0) && !hy_df_lt(t1, tg)) || done_lane;
        if (!avail) break;
        const double hd = hy_df_sub(tg, tstart).hi;
)HIP";
    if (sec == nullptr) {
        src << R"HIP(        for (unsigned v = 0; v < HY_DIM; ++v) {
            const double *c = a.tc + (u64)v * (HY_ORDER + 1u) * N + i;
)HIP" << dense_row_text
            << R"HIP(            a.out[((u64)g * HY_DIM + v) * N + i] = res;
        }
)HIP";
    } else {
        // The rows the observables read, in the order of the plain loop, then the section. The loop over the rows runs over
        // the table hy_obs_rows with the body of the plain loop, text for text (dense_row_text): the compiler makes of the
        // inner loop what it makes of it in the plain kernel - in particular it does or does not unroll it completely, which
        // decides whether its first iteration is folded (comp = 0) and with that the last bits of the sample. Staged: a loop,
        // the samples go to the staging buffer. Registers: the loop over the rows is unrolled into the named values xs[j];
        // a scheduling barrier behind every row keeps the loads of one row in flight, not those of all of them (HY_ORDER + 1
        // coefficients per row: 1 512 VGPRs for the 36 rows of the outer Solar System).
        // The coefficients do not depend on the grid point: the empty asm statements on their base address and on the stride
        // keep the loads and the scalar offsets inside the iteration of the while loop (hoisted out of it they are all alive
        // at once again).
        if (!sec->stats.empty()) {
            // Grid statistics: what is folded cannot be taken back - the first merge of a sweep is preceded by the copy of
            // the lane's accumulators which hy_grid_unsample restores. Ahead of the samples: nothing of the point is alive
            // yet. (The grid index of a lane starts at 1: row 0 is hy_grid_obs0's, and the start branch of the section goes.)
            src << R"HIP(        if (!shadowed) {
            for (unsigned s = 0; s < HY_NSLOT; ++s) out0[(u64)(HY_NSLOT + s) * N] = out0[(u64)s * N];
            shadowed = true;
        }
        __builtin_assume(g != 0u);
)HIP";
        }
        src << "        const double *tcb = tc0;\n        asm volatile(\"\" : \"+v\"(tcb));\n";
        src << "        u64 Ns = N;\n        asm volatile(\"\" : \"+s\"(Ns));\n";
        if (!sec->staged) {
            src << "        double xs[" << (sec->reads.empty() ? "1" : "HY_NROWS") << "];\n#pragma unroll\n";
        }
        src << R"HIP(        for (unsigned j = 0; j < HY_NROWS; ++j) {
            const unsigned v = hy_obs_rows[j];
            // (This N shadows the kernel's on purpose: the shared body below says N, and here it must be the stride Ns.)
            const u64 N = Ns;
            const double *c = tcb + (u64)v * (HY_ORDER + 1u) * N;
)HIP" << dense_row_text;
        if (sec->staged) {
            src << "            stg[(u64)v * N] = res;\n        }\n";
        } else {
            src << "            xs[j] = res;\n            __builtin_amdgcn_sched_barrier(0);\n        }\n";
        }
        src << "        " << grid_obs_call(*sec, !sec->merges() ? "out0" : "a.out", "stg", "xs", "g", "tg.hi");
    }
    src << R"HIP(        ++g;
    }
    if (retire) g = ng;
    a.gidx[i] = g;
    // (The next grid time of the lane: the steps which do not reach it need not store their Taylor coefficients.)
    if (a.next_tg != nullptr) {
        a.next_tg[i] = (g < ng) ? a.grid[(u64)g * N + i] : ((a.t_dir[i] != 0) ? __builtin_inf() : -__builtin_inf());
    }
    // Limit of the next step.
    hy_df m; m.lo = 0.0;
    double lim;
    if (a.t_dir[i] != 0) { m.hi = a.mdt[i]; lim = hy_df_lt(rem, m) ? rem.hi : m.hi; }
    else { m.hi = -a.mdt[i]; lim = hy_df_lt(m, rem) ? rem.hi : m.hi; }
    a.lim[i] = retire ? 0.0 : lim;
    hy_count(a.counters, g < ng);
}
)HIP";
    if (sec != nullptr && !sec->stats.empty()) {
        // (The lock-step sweeps in which this kernel runs retire nobody: a grid index which moved is a lane which merged, and
        // a lane which merged has made its copy.)
        src << R"HIP(
// A sweep in which a lane went non-finite: the reference leaves its loop right after that step, before the dense output of
// the step (src/taylor_adaptive_batch.cpp:1962-1968) - the lanes which merged grid points in hy_grid_post just now get back
// the accumulators they had before. Nothing of the size of the grid is written.
extern "C" __global__ void __launch_bounds__(256) hy_grid_unsample(const hy_grid_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (i >= N) return;
    if (a.gidx_prev[i] < a.gidx[i]) {
        for (unsigned s = 0; s < HY_NSLOT; ++s) a.out[(u64)s * N + i] = a.out[(u64)(HY_NSLOT + s) * N + i];
    }
}
)HIP";
    } else if (sec != nullptr && sec->merges()) {
        // (Ensemble statistics: the records are restored by the host from its copy, there is no hy_grid_unsample.)
        src << R"HIP(
// Row 0 into the records: the observables of the current state at the first grid time (at the start of the call and again
// after a rollback, into records in their start state).
)HIP";
    } else {
        src << R"HIP(
// A sweep in which a lane went non-finite: the reference leaves its loop right after that step, before the dense output of
// the step (src/taylor_adaptive_batch.cpp:1962-1968; the samples of a step are taken at the top of the NEXT iteration,
// :1800-1871) - the samples hy_grid_post has just taken in the other lanes are NaN again.
extern "C" __global__ void __launch_bounds__(256) hy_grid_unsample(const hy_grid_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (i >= N) return;
    const unsigned g1 = a.gidx[i];
    for (unsigned g = a.gidx_prev[i]; g < g1; ++g) {
        for (unsigned v = 0; v < )HIP" << ncol << R"HIP(; ++v) {
            a.out[((u64)g * )HIP" << ncol << R"HIP( + v) * N + i] = __builtin_nan("");
        }
    }
}
)HIP";
    }
    if (sec != nullptr) {
        if (sec->merges()) {
        } else if (!sec->stats.empty()) {
            src << "\n// The start of the accumulators: the observables of the current state at the first grid time (at the start of "
                   "the call and\n// again after a rollback).\n";
        } else {
            src << R"HIP(
// Row 0 of the output: the observables of the current state at the first grid time (at the start of the call and again
// after a rollback).
)HIP";
        }
        src << R"HIP(extern "C" __global__ void __launch_bounds__(256) hy_grid_obs0(const hy_grid_args a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (i >= N) return;
)HIP";
        if (sec->staged) {
            src << "    double *stg = a.stage + i;\n";
        } else {
            src << "    double xs[" << (sec->reads.empty() ? "1" : "HY_NROWS") << "];\n";
        }
        std::size_t n_obs0 = 0;
        for (const auto r : sec->reads) {
            if (sec->staged) {
                src << "    stg[(u64)" << r << "u * N] = a.state[(u64)" << r << "u * N + i];\n";
            } else {
                src << "    xs[" << n_obs0++ << "] = a.state[(u64)" << r << "u * N + i];\n";
            }
        }
        src << "    " << grid_obs_call(*sec, !sec->merges() ? "a.out + i" : "a.out", "stg", "xs", "0u", "a.grid[i]") << "}\n";
    }
    return src.str();
}

void tab_core::impl::ensure_grid_mod() const
{
    if (!grid_mod) {
        grid_mod = std::make_unique<aux_module>(hiprtc_compile_source(make_grid_source(order, dim, high_accuracy)), device);
    }
}

} // namespace heyoka_amd::detail
