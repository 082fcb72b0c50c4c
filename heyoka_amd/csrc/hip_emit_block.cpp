// HIP code generation, "block" mode: one ODE system per workgroup.
//
// Target: decompositions with many isomorphic nonlinear clusters, e.g. model::nbody(64) (2016 body pairs,
// 18 663 u variables; BASELINE config 5), where a system cannot live in one wavefront: the jets of the
// clusters (2016 x 5 x 20 doubles = 1.6 MB) exceed the register file *and* the LDS of a compute unit.
// With one lane per system (table mode) the tape is 3 MB per lane, the ensemble exposes only one
// wavefront per SIMD and every convolution term is an uncoalesced-by-design HBM access.
//
// Here the 256 lanes of a workgroup cooperate on one system at a time:
//  * cluster phase (order k): lane = cluster (strided over the clusters). The lane loads the lower-order
//    coefficients of the cluster's "stored" members from a per-workgroup tape in global memory, laid out
//    tape[(member * order + m) * n_clusters + cluster] so that the lanes of a wave read consecutive
//    addresses (fully coalesced 512 B requests; the tape of the systems in flight is L2 / MALL sized),
//    evaluates the cluster's recurrences with the same node emitters as the other modes, stores the new
//    coefficients and publishes the cluster outputs to an LDS slab;
//  * glue phases: lane = glue node (sums / differences / scalings of current-order values), grouped by
//    dependency level and shape, operands and results in the LDS slab, slots from tables in global memory
//    (coalesced, L2-resident, shared by all the workgroups);
//  * state-variable recursion x^[k+1] = rhs^[k] / (k + 1), lane = state variable; the jets of the state
//    variables go to a small per-workgroup array in global memory for the final Horner / compensated
//    update, again with lane = state variable;
//  * infinity norms for the step-size selector: wave shuffles + one LDS exchange.
// Workgroups are persistent and pull systems from the device-side work queue.
//
// Reference semantics of every phase as in the other modes:
// taylor_compute_jet (src/taylor_02.cpp:1339-1418), taylor_determine_h (src/taylor_00.cpp:102-273),
// taylor_run_multihorner / taylor_run_ceval (:279-460), step / propagate semantics
// (src/taylor_adaptive_batch.cpp:632-727, :1137-1534).
//
// The generator is one object per call (hip_emit_block_gen.hpp: the stages, the data they share, the list of the switches
// of HEYOKA_AMD_BLOCK_OPTS); this file holds the driver and every stage but the pair phase (hip_emit_block_pair.cpp).
#include <algorithm>
#include <cstdlib>
#include <map>
#include <numeric>
#include <set>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "hip_emit_block_gen.hpp"
#include "logging.hpp"

namespace heyoka_amd
{

namespace block_detail
{

using namespace cluster_detail;

block_switches block_switches::parse(const std::string &list)
{
    std::map<std::string, int> given;
    for (std::size_t pos = 0; pos <= list.size();) {
        const auto end = std::min(list.find_first_of(",:", pos), list.size());
        const auto item = list.substr(pos, end - pos);
        pos = end + 1u;
        const auto eq = item.find('=');
        // (The workgroup size has no meaning without its value: a bare "bs" is no item.)
        if (item.empty() || (eq == std::string::npos && item == "bs")) {
            continue;
        }
        given.emplace(item.substr(0, eq), eq == std::string::npos ? 1 : std::atoi(item.c_str() + eq + 1u));
    }
    block_switches sw;
    const auto get = [&given](const char *name, auto &dst) {
        if (const auto it = given.find(name); it != given.end()) {
            dst = static_cast<std::remove_reference_t<decltype(dst)>>(it->second);
        }
    };
    get("bs", sw.bs);
    get("nopad", sw.nopad);
    get("perm", sw.perm);
    get("licm", sw.licm);
    get("M", sw.M);
    get("G", sw.G);
    get("D", sw.D);
    get("hand", sw.hand);
    get("hoist", sw.hoist);
    get("keepdz", sw.keepdz);
    get("nopp", sw.nopp);
    get("reg_high", sw.reg_high);
    get("div", sw.div);
    get("split", sw.split);
    get("xpf", sw.xpf);
    get("unpacked", sw.unpacked);
    get("noglueperm", sw.noglueperm);
    get("nofuse", sw.nofuse);
    get("dbuf", sw.dbuf);
    get("exp", sw.exp);
    return sw;
}

void block_tables::emit_utbl(const std::string &name, const std::vector<std::uint32_t> &v)
{
    utbl_list.emplace_back(name, std::max<std::size_t>(v.size(), 1u));
    tbl << "__device__ const " << ut << " __attribute__((aligned(16))) " << name << "[" << std::max<std::size_t>(v.size(), 1u) << "] = {";
    for (const auto x : v) {
        tbl << x << ",";
    }
    tbl << "};\n";
}

void block_tables::emit_dtbl(const std::string &name, const std::vector<double> &v)
{
    tbl << "__device__ const double " << name << "[" << std::max<std::size_t>(v.size(), 1u) << "] = {";
    for (const auto x : v) {
        tbl << fp_literal(x) << ",";
    }
    tbl << "};\n";
}

block_gen::block_gen(const taylor_program &p_, const emit_options &opts_, emit_refusal &why_not_)
    : p(p_), opts(opts_), why_not(why_not_), sw(block_switches::parse(opts_.dev.block_opts)), n_eq(p_.n_eq), order(opts_.order),
      e(p_, opts_.order), os(e.os)
{
}

// ---- stage 1: the cluster plan, the slab layout, the (preliminary) workgroup size, the counts ----
bool block_gen::plan()
{
    plan_limits lim;
    lim.max_clusters = 1u << 20;
    lim.jets_in_registers = false;
    lim.absorb_linear = !opts.block_no_absorb;
    why_not = make_plan(p, order, pl, lim);
    if (!why_not.empty()) {
        return false;
    }
    pad_output_blocks();
    nc = static_cast<std::uint32_t>(pl.clusters.size());
    ncp = (nc + 63u) / 64u * 64u;
    n_ext = static_cast<std::uint32_t>(pl.ext_u[0].size());
    n_out = static_cast<std::uint32_t>(pl.out_pos.size());
    n_cst = static_cast<std::uint32_t>(pl.cst_pos.size());
    n_sto = static_cast<std::uint32_t>(pl.stored_pos.size());
    n_slots = pl.n_slots;
    wide = n_slots > 65535u;
    // Workgroup size: 256 lanes = one wavefront per SIMD with the whole register file (512 VGPRs) for the
    // history of the cluster being processed.
    // Small cluster counts: do not park lanes (several smaller workgroups fit on a compute unit).
    // (Switch bs: A/B harness. The pair phase may still go to 512 lanes: pair_phase_applicable().)
    set_workgroup_size(sw.bs ? static_cast<std::uint32_t>(*sw.bs) : (nc <= 128u ? 128u : 256u), n_eq);

    // Registers: the history of the stored members is loaded at every order.
    if (static_cast<std::uint64_t>(n_sto) * order * 2u > 440u) {
        why_not = "the jets of a cluster do not fit in the register file";
        return false;
    }
    return true;
}

// Slots of the exported cluster members: output-major blocks of n_clusters slots each. When the number of clusters is a
// multiple of the 32 bank pairs of LDS (2016 for nbody(64)), the three products of a pair sit in ONE bank, and so do
// the operands of the sums of the three coordinates of a body, which the glue gathers on adjacent lanes: one slot of
// padding between the blocks (an odd distance). (Switch nopad: A/B harness.)
void block_gen::pad_output_blocks()
{
    if (pl.classes.size() <= 1u && pl.clusters.size() % 2u == 0u && pl.out_pos.size() > 1u && !sw.nopad) {
        const auto ncl = static_cast<int>(pl.clusters.size()), nout = static_cast<int>(pl.out_pos.size());
        const auto first = static_cast<int>(n_eq), last = first + ncl * nout;
        bool layout_ok = true;
        for (int c = 0; c < ncl && layout_ok; ++c) {
            for (int q = 0; q < nout; ++q) {
                layout_ok = layout_ok && pl.slot_of[pl.clusters[static_cast<std::size_t>(c)][pl.out_pos[static_cast<std::size_t>(q)]]] == first + q * ncl + c;
            }
        }
        if (layout_ok) {
            for (auto &sl : pl.slot_of) {
                if (sl >= last) {
                    sl += nout - 1;
                } else if (sl >= first) {
                    sl += (sl - first) / ncl;
                }
            }
            pl.n_slots += static_cast<std::uint32_t>(nout - 1);
        }
    }
}

// ---- stage 2: which members go through the tape ----
// Stored members which are linear functions of external inputs only (e.g. the coordinate differences of
// an N-body pair) are not written to the tape: their lower-order coefficients are recomputed from the
// jets of the external inputs, which are kept in LDS (ejet[m * n_ej + e]). This removes 3 of the 5 tape
// streams of the N-body clusters.
bool block_gen::input_jets()
{
    recomp.assign(n_sto, 0);
    ext_used.assign(n_ext, 0);
    {
        std::map<std::uint32_t, std::uint32_t> ext_pos;
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            ext_pos[pl.ext_u[0][x]] = x;
        }
        for (std::uint32_t s = 0; s < n_sto; ++s) {
            const auto &n = p.nodes[t0()[pl.stored_pos[s]] - n_eq];
            bool ok = (n.kind == func_kind::sub || n.kind == func_kind::sum
                       || (n.kind == func_kind::prod && n.args.size() == 2u && !is_var(n.args[0])));
            bool any_var = false;
            for (const auto &o : n.args) {
                if (is_var(o)) {
                    any_var = true;
                    ok = ok && ext_pos.count(o.idx) != 0u;
                }
            }
            if (ok && any_var) {
                recomp[s] = 1;
                for (const auto &o : n.args) {
                    if (is_var(o)) {
                        ext_used[ext_pos[o.idx]] = 1;
                    }
                }
            }
        }
        // (Jets in the order of the external inputs of the template, within one input by ascending slot: the layout does not
        // depend on the order of the clusters.)
        std::map<std::uint32_t, std::uint32_t> slot_to_ej;
        ej_index.assign(static_cast<std::size_t>(n_ext) * nc, 0u);
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            if (ext_used[x] == 0) {
                continue;
            }
            std::set<std::uint32_t> fresh;
            for (std::uint32_t c = 0; c < nc; ++c) {
                const auto slot = static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[c][x]]);
                if (slot_to_ej.count(slot) == 0u) {
                    fresh.insert(slot);
                }
            }
            for (const auto slot : fresh) {
                slot_to_ej.emplace(slot, static_cast<std::uint32_t>(ej_slots.size()));
                ej_slots.push_back(slot);
            }
            for (std::uint32_t c = 0; c < nc; ++c) {
                ej_index[static_cast<std::size_t>(x) * nc + c] = slot_to_ej[static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[c][x]])];
            }
        }
        if (!ej_slots.empty() && nc >= 64u && sw.perm) {
            permute_clusters();
        }
    }
    n_ej = static_cast<std::uint32_t>(ej_slots.size());
    const auto lds_for = [this](std::uint32_t nej) {
        return static_cast<std::uint64_t>(n_slots) * 8u + static_cast<std::uint64_t>(nej) * (order - 1u) * 8u + 128u;
    };
    if (lds_for(n_ej) > 150u * 1024u) {
        // No room for the jets of the external inputs: everything goes through the tape.
        std::fill(recomp.begin(), recomp.end(), 0);
        std::fill(ext_used.begin(), ext_used.end(), 0);
        ej_slots.clear();
        n_ej = 0;
    }
    if (lds_for(n_ej) > 150u * 1024u) {
        why_not = "the exchange slab does not fit in LDS";
        return false;
    }
    // Tape rows: only the members which are not recomputed.
    tape_row.assign(n_sto, 0u);
    n_tape = 0;
    for (std::uint32_t s = 0; s < n_sto; ++s) {
        if (recomp[s] == 0) {
            tape_row[s] = n_tape++;
        }
    }
    for (const auto &d : p.sv_defs) {
        if (d.type == operand::kind::uvar && pl.slot_of[d.idx] < 0) {
            why_not = "state variable definition without a slot";
            return false;
        }
    }
    return true;
}

// Order of the clusters (round 6): lane l of a wavefront reads the jets of the inputs of ITS cluster from LDS - 64-bit
// reads, served 32 lanes at a time, one cycle when the addresses of a group of 32 lanes fall into distinct banks
// (or coincide). In the order of the decomposition (pairs of an N-body system: body-major) a group of 32 straddles
// the boundary between two bodies and its partners collide: 1.24 cycles per group on nbody(64), a quarter of the
// LDS cycles of the kernel. The switch perm deals the clusters greedily into groups of 32 whose inputs are
// conflict-free input by input (1.01 on nbody(64)) - MEASURED: 1.506e6 against 1.525e6 system-steps/s in the order
// of the decomposition (profiles/r06_nbody64_experiments.log): the conflicts of these reads are not what binds;
// the order of the decomposition stays the default.
void block_gen::permute_clusters()
{
    std::vector<std::uint32_t> rem(nc), order_;
    std::iota(rem.begin(), rem.end(), 0u);
    order_.reserve(nc);
    while (!rem.empty()) {
        std::vector<std::uint32_t> grp, keep;
        std::vector<std::map<std::uint32_t, std::uint32_t>> bank(n_ext);
        for (const auto c : rem) {
            bool ok = grp.size() < 32u;
            for (std::uint32_t x = 0; x < n_ext && ok; ++x) {
                if (ext_used[x] != 0) {
                    const auto a = ej_index[static_cast<std::size_t>(x) * nc + c];
                    const auto it = bank[x].find(a % 32u);
                    ok = it == bank[x].end() || it->second == a;
                }
            }
            if (ok) {
                grp.push_back(c);
                for (std::uint32_t x = 0; x < n_ext; ++x) {
                    if (ext_used[x] != 0) {
                        const auto a = ej_index[static_cast<std::size_t>(x) * nc + c];
                        bank[x][a % 32u] = a;
                    }
                }
            } else {
                keep.push_back(c);
            }
        }
        std::size_t taken = 0;
        while (grp.size() < 32u && taken < keep.size()) {
            grp.push_back(keep[taken++]);
        }
        keep.erase(keep.begin(), keep.begin() + static_cast<std::ptrdiff_t>(taken));
        order_.insert(order_.end(), grp.begin(), grp.end());
        rem.swap(keep);
    }
    // new position -> old cluster: apply to everything indexed by the cluster.
    std::vector<std::uint32_t> new_of(nc);
    for (std::uint32_t i = 0; i < nc; ++i) {
        new_of[order_[i]] = i;
    }
    const auto permute = [&order_, n = nc](auto &v) {
        if (v.size() == n) {
            const auto w = v;
            for (std::uint32_t i = 0; i < n; ++i) {
                v[i] = w[order_[i]];
            }
        }
    };
    permute(pl.clusters);
    permute(pl.ext_u);
    permute(pl.cst_val);
    permute(pl.par_idx);
    for (auto &c : pl.cluster_of) {
        if (c >= 0) {
            c = static_cast<int>(new_of[static_cast<std::uint32_t>(c)]);
        }
    }
    for (auto &cls : pl.classes) {
        for (auto &m : cls.members) {
            m = new_of[m];
        }
    }
    auto ej2 = ej_index;
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        for (std::uint32_t i = 0; i < nc; ++i) {
            ej2[static_cast<std::size_t>(x) * nc + i] = ej_index[static_cast<std::size_t>(x) * nc + order_[i]];
        }
    }
    ej_index.swap(ej2);
}

// ---- stage 3: the tables both cluster phases read ----
void block_gen::base_tables()
{
    ut = wide ? "unsigned" : "unsigned short";
    {
        std::vector<std::uint32_t> v(static_cast<std::size_t>(n_ext) * nc);
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            for (std::uint32_t c = 0; c < nc; ++c) {
                v[static_cast<std::size_t>(x) * nc + c] = static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[c][x]]);
            }
        }
        emit_utbl("hy_ext", v);
        v.assign(static_cast<std::size_t>(n_out) * nc, 0u);
        for (std::uint32_t x = 0; x < n_out; ++x) {
            for (std::uint32_t c = 0; c < nc; ++c) {
                v[static_cast<std::size_t>(x) * nc + c]
                    = static_cast<std::uint32_t>(pl.slot_of[pl.clusters[c][pl.out_pos[x]]]);
            }
        }
        emit_utbl("hy_out", v);
        std::vector<double> dv(static_cast<std::size_t>(n_cst) * nc);
        for (std::uint32_t x = 0; x < n_cst; ++x) {
            for (std::uint32_t c = 0; c < nc; ++c) {
                dv[static_cast<std::size_t>(x) * nc + c] = pl.cst_val[c][x];
            }
        }
        emit_dtbl("hy_cst", dv);
        emit_utbl("hy_extj", n_ej != 0u ? ej_index : std::vector<std::uint32_t>{});
        emit_utbl("hy_ejs", ej_slots);
    }
    // Glue groups: per argument a table of slots (variables) or of values (non-structural numbers).
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &grp = pl.groups[g];
        const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
        for (std::size_t a = 0; a < n0.args.size(); ++a) {
            const auto name = "hy_g" + std::to_string(g) + "_a" + std::to_string(a);
            if (is_var(n0.args[a])) {
                std::vector<std::uint32_t> v;
                for (const auto u : grp.nodes) {
                    v.push_back(static_cast<std::uint32_t>(pl.slot_of[p.nodes[u - n_eq].args[a].idx]));
                }
                emit_utbl(name, v);
            } else if (n0.args[a].type == operand::kind::num) {
                std::vector<double> v;
                for (const auto u : grp.nodes) {
                    v.push_back(p.nodes[u - n_eq].args[a].value);
                }
                emit_dtbl(name, v);
            }
        }
        std::vector<std::uint32_t> v;
        for (const auto u : grp.nodes) {
            v.push_back(static_cast<std::uint32_t>(pl.slot_of[u]));
        }
        emit_utbl("hy_g" + std::to_string(g) + "_o", v);
    }
    // State-variable definitions: kind 0 = u variable (slot), 1 = number, 2 = parameter.
    {
        std::vector<std::uint32_t> kind(n_eq), idx(n_eq);
        std::vector<double> val(n_eq, 0.);
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            const auto &d = p.sv_defs[i];
            if (d.type == operand::kind::uvar) {
                kind[i] = 0;
                idx[i] = static_cast<std::uint32_t>(pl.slot_of[d.idx]);
            } else if (d.type == operand::kind::num) {
                kind[i] = 1;
                val[i] = d.value;
            } else {
                kind[i] = 2;
                idx[i] = d.idx;
            }
        }
        emit_utbl("hy_sv_kind", kind);
        emit_utbl("hy_sv_idx", idx);
        emit_dtbl("hy_sv_val", val);
    }
}

// ---- stage 4: is the cluster phase the pair phase ("v2 cluster phase", hip_emit_block_pair.cpp)? ----
// The order loop is ROLLED and the rounds of a lane (its n_iter clusters) are unrolled, so that the coefficients of
// order < M of the two members with a recurrence on themselves (r^2 and its power) stay in REGISTERS for the whole
// step (2 * M doubles per cluster of the lane); the convolutions are evaluated as index pairs (i, k - i), i < k - i:
// the low index from the registers (or, for M <= i, from the tape), the high index from the tape - every tape row
// >= M is read once per order instead of every row, and the rows just written are the ones read next (L2).
bool block_gen::pair_phase_applicable()
{
    detect_pair_pattern(p, pl, pp);
    T = (order - 1u) / 2u + 1u;
    const bool applicable = [this]() {
        if (!opts.dev.block_v2) {
            return false;
        }
        if (!pp.ok || pp.sc != -1 || pp.rx[0] != -1 || pp.rx[1] != -1 || pp.rx[2] != -1 || n_cst != 0u
            || !pl.par_pos.empty() || pl.glue_has_par || wide || pl.cluster_level != 1u || n_ej == 0u || n_tape != 2u
            || n_out != 3u || order < 6u || p.n_par != 0u) {
            detail::log_message(log_level::debug,
                                "block mode, v2 cluster phase not applicable: pair pattern " + std::to_string(pp.ok) + ", scaling "
                                    + std::to_string(pp.sc) + ", reactions " + std::to_string(pp.rx[0]) + ", constants "
                                    + std::to_string(n_cst) + ", wide " + std::to_string(wide) + ", cluster level "
                                    + std::to_string(pl.cluster_level) + ", external jets " + std::to_string(n_ej) + ", tape members "
                                    + std::to_string(n_tape) + ", outputs " + std::to_string(n_out));
            return false;
        }
        // (The rounds per lane with one wavefront per SIMD: n_iter of the preliminary workgroup size.)
        if (static_cast<std::uint64_t>(n_ej) * order * 8u >= 65536u || n_iter > 16u) {
            return false;
        }
        for (const auto c : constant_uvars(p)) {
            if (c != 0) {
                return false;
            }
        }
        // External inputs: state variables (their order-k values are recorded by the state recursion).
        for (std::uint32_t c = 0; c < nc; ++c) {
            for (std::uint32_t x = 0; x < n_ext; ++x) {
                const auto u = pl.ext_u[c][x];
                if (u >= n_eq || pl.slot_of[u] != static_cast<int>(u)) {
                    return false;
                }
            }
        }
        // Glue: nodes whose order-k rule is the same for every k >= 1.
        for (const auto &grp : pl.groups) {
            const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
            bool ok = false;
            if (n0.kind == func_kind::sum || n0.kind == func_kind::sub) {
                ok = true;
            } else if (n0.kind == func_kind::prod && n0.args.size() == 2u && n0.args[0].type == operand::kind::num
                       && is_var(n0.args[1])) {
                ok = true;
            }
            if (!ok) {
                return false;
            }
        }
        return true;
    }();
    // Two wavefronts per SIMD for the v2 cluster phase with more than four rounds per lane (round 6): 512 lanes with 256
    // registers each. With eight rounds on one wavefront per SIMD the kernel was bound by the ISSUE of its single
    // wavefront (8.5 cycles per instruction by the counters: 30 % VALU, 13 % LDS, 5 % memory, the rest waiting); HBM bytes,
    // LDS reads and tape loads of the slots each removed in turn gained 11 ... 13 % only (profiles/r06_nbody64_experiments.log).
    // With a second wavefront the ping-pong of the LDS operands is not needed (the other wavefront covers the latency; its
    // registers go to the rows in registers), groups of two rounds, tape loads two slots ahead: nbody(64) 1.42e6 -> 1.52e6.
    if (applicable && bs == 256u && nc > 1024u && !sw.bs) {
        set_workgroup_size(512, n_eq);
        two_waves = true;
    }
    return applicable;
}

// ---- the step body: what both cluster phases begin with ----
void block_gen::begin_body()
{
    for (std::uint32_t x = 0; x < n_cst; ++x) {
        const auto [q, a] = pl.cst_pos[x];
        e.numpar_override[&p.nodes[t0()[q] - n_eq].args[a]] = "ccst" + std::to_string(x);
    }
    os << "double m0 = 0.0, mo = 0.0, mom1 = 0.0;\n";
    // Order 0: the state is already in slab[0 .. n_eq) and sjet[0 .. n_eq) (see the module text).
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        os << "{ const unsigned i = tid + " << r * bs << "u; if (i < " << n_eq
           << "u) m0 = hy_max(m0, fabs(slab[i])); }\n";
    }
}

// ---- stage 5: the generic cluster phase, orders unrolled ----
// Cluster phase at order k: a rolled loop over the clusters of the lane; everything a round needs (slot indices,
// per-cluster constants, tape history) is loaded at the top of the round.
// (Software pipelining of these loads - the indices / constants, or the tape history as well, requested one round ahead -
// was measured on an MI355X (nbody64, 65 536 systems): 8.4e5 without, 5.0e5 system-steps/s with the history - the
// loop-carried copies of the history push the kernel over the 512-VGPR budget and the spill traffic
// costs more than the latency it hides. Removed.)
void block_gen::emit_cluster(std::uint32_t k)
{
    constexpr std::uint32_t sched_every = 4;
    if (n_ej != 0u && k + 1u < order) {
        // Record the order-k coefficients of the external inputs (read back from order k + 1 on).
        os << "for (unsigned e = tid; e < " << n_ej << "u; e += " << bs << "u) ejet["
           << static_cast<std::uint64_t>(k) * n_ej << "u + e] = slab[hy_ejs[e]];\n";
    }
    // Names of the per-cluster loads: (variable name, type, load expression in terms of `cw`).
    struct load {
        std::string name, type, expr;
    };
    std::vector<load> loads;
    for (std::uint32_t x = 0; x < n_cst; ++x) {
        loads.push_back({"ccst" + std::to_string(x), "double",
                         "hy_cst[" + std::to_string(static_cast<std::uint64_t>(x) * nc) + "u + cw]"});
    }
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        loads.push_back({"ie" + std::to_string(x), "unsigned",
                         "hy_ext[" + std::to_string(static_cast<std::uint64_t>(x) * nc) + "u + cw]"});
    }
    for (std::uint32_t x = 0; x < n_out; ++x) {
        loads.push_back({"io" + std::to_string(x), "unsigned",
                         "hy_out[" + std::to_string(static_cast<std::uint64_t>(x) * nc) + "u + cw]"});
    }
    if (n_ej != 0u && k > 0u) {
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            if (ext_used[x] != 0) {
                loads.push_back({"ej" + std::to_string(x), "unsigned",
                                 "hy_extj[" + std::to_string(static_cast<std::uint64_t>(x) * nc) + "u + cw]"});
            }
        }
    }
    for (std::uint32_t s = 0; s < n_sto; ++s) {
        if (recomp[s] != 0) {
            continue;
        }
        const auto u = t0()[pl.stored_pos[s]];
        for (std::uint32_t m = 0; m < k; ++m) {
            const auto nm = "h" + std::to_string(s) + "_" + std::to_string(m);
            loads.push_back({nm, "double",
                             "tape[" + std::to_string((static_cast<std::uint64_t>(tape_row[s]) * order + m) * ncp)
                                 + "u + cw]"});
            e.val(u, m) = nm;
        }
    }
    // (The idle lanes of a partial last round replicate the last cluster and do not write anything. The scope with the
    // unused `cc` is what is left of the prologue of the pipelined loads: the text of the kernels is pinned.)
    os << "{\n";
    os << "unsigned c = tid;\n";
    os << "{\nconst unsigned cc = c < " << nc << "u ? c : " << nc - 1u << "u;\n";
    os << "}\n";
    os << "#pragma nounroll\n";
    os << "for (unsigned it = 0; it < " << n_iter << "u; ++it, c += " << bs << "u) {\n";
    os << "const bool live = c < " << nc << "u;\n";
    os << "const unsigned cw = live ? c : " << nc - 1u << "u;\n";
    for (const auto &l : loads) {
        os << "const " << l.type << " " << l.name << " = " << l.expr << ";\n";
    }
    // Lower-order coefficients recomputed from the LDS jets of the external inputs.
    if (n_ej != 0u && k > 0u) {
        for (std::uint32_t m = 0; m < k; ++m) {
            for (std::uint32_t x = 0; x < n_ext; ++x) {
                if (ext_used[x] != 0) {
                    e.val(pl.ext_u[0][x], m)
                        = e.def("ejet[" + std::to_string(static_cast<std::uint64_t>(m) * n_ej) + "u + ej"
                                + std::to_string(x) + "]");
                }
            }
            for (std::uint32_t s = 0; s < n_sto; ++s) {
                if (recomp[s] != 0) {
                    e.node(t0()[pl.stored_pos[s]] - n_eq, m);
                }
            }
            // NOTE: without a fence the scheduler hoists all the LDS reads of the inputs' jets to the top
            // (2 * 3 * k live doubles on top of the history itself): hundreds of spilled registers.
            if (m % sched_every == sched_every - 1u) {
                os << "__builtin_amdgcn_sched_barrier(0);\n";
            }
        }
        os << "__builtin_amdgcn_sched_barrier(0);\n";
    }
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        e.val(pl.ext_u[0][x], k) = e.def("slab[ie" + std::to_string(x) + "]");
    }
    for (const auto u : t0()) {
        e.node(u - n_eq, k);
    }
    os << "if (live) {\n";
    if (k + 1u < order) {
        for (std::uint32_t s = 0; s < n_sto; ++s) {
            if (recomp[s] == 0) {
                os << "tape[" << (static_cast<std::uint64_t>(tape_row[s]) * order + k) * ncp
                   << "u + cw] = " << e.val(t0()[pl.stored_pos[s]], k) << ";\n";
            }
        }
    }
    for (std::uint32_t x = 0; x < n_out; ++x) {
        os << "slab[io" << x << "] = " << e.val(t0()[pl.out_pos[x]], k) << ";\n";
    }
    os << "}\n";
    os << "}\n}\n";
}

// Glue group at order k: branch-free rounds (clamped node index, the result of an idle lane goes to a dummy
// slot), so that all the groups of a level form one basic block and their table / LDS loads overlap.
void block_gen::emit_glue_group(std::size_t g, std::uint32_t k)
{
    const auto &grp = pl.groups[g];
    const auto rep = grp.nodes[0];
    const auto &n0 = p.nodes[rep - n_eq];
    const auto gn = "hy_g" + std::to_string(g);
    const auto ng = static_cast<std::uint32_t>(grp.nodes.size());
    for (std::uint32_t r = 0; r * bs < ng; ++r) {
        os << "{\nconst unsigned jr = tid + " << r * bs << "u;\n";
        const bool partial = (r + 1u) * bs > ng;
        if (partial) {
            os << "const bool ok = jr < " << ng << "u;\nconst unsigned j = ok ? jr : " << ng - 1u << "u;\n";
        } else {
            os << "const unsigned j = jr;\n";
        }
        const auto saved = e.numpar_override;
        std::vector<std::pair<std::uint32_t, std::string>> saved_vals;
        for (std::size_t a = 0; a < n0.args.size(); ++a) {
            const auto &o = n0.args[a];
            if (is_var(o)) {
                const auto nm = e.def("slab[" + gn + "_a" + std::to_string(a) + "[j]]");
                saved_vals.emplace_back(o.idx, e.val(o.idx, k));
                e.val(o.idx, k) = nm;
            } else if (o.type == operand::kind::num) {
                e.numpar_override[&o] = gn + "_a" + std::to_string(a) + "[j]";
            }
        }
        if (n0.kind == func_kind::prod && n0.args[0].type == operand::kind::num && n0.args[0].value == -1.) {
            e.numpar_override.erase(&n0.args[0]);
        }
        e.node(rep - n_eq, k);
        if (partial) {
            os << "slab[ok ? (unsigned)" << gn << "_o[j] : " << n_slots << "u] = " << e.val(rep, k) << ";\n";
        } else {
            os << "slab[" << gn << "_o[j]] = " << e.val(rep, k) << ";\n";
        }
        for (auto it = saved_vals.rbegin(); it != saved_vals.rend(); ++it) {
            e.val(it->first, k) = it->second;
        }
        e.numpar_override = saved;
        os << "}\n";
    }
}

void block_gen::generic_body()
{
    for (std::uint32_t k = 0; k < order; ++k) {
        os << "// ---- order " << k << " ----\n";
        for (std::uint32_t lev = 1; lev <= pl.max_level; ++lev) {
            if (lev == pl.cluster_level) {
                emit_cluster(k);
            }
            for (std::size_t g = 0; g < pl.groups.size(); ++g) {
                if (pl.groups[g].level == lev) {
                    emit_glue_group(g, k);
                }
            }
            sync();
        }
        // State-variable recursion (src/taylor_02.cpp:245-287): read rhs^[k], sync, write x^[k+1].
        os << "{\n";
        for (std::uint32_t r = 0; r < sv_rounds; ++r) {
            os << "double xn" << r << " = 0.0;\n";
            os << "{ const unsigned i = tid + " << r * bs << "u; if (i < " << n_eq << "u) {\n";
            os << "const unsigned kd = hy_sv_kind[i];\n";
            os << "if (kd == 0u) xn" << r << " = slab[hy_sv_idx[i]] / " << fp_literal(static_cast<double>(k + 1u))
               << ";\n";
            if (k == 0u) {
                os << "else if (kd == 1u) xn" << r << " = hy_sv_val[i];\n";
                os << "else xn" << r << " = a.pars[(u64)hy_sv_idx[i] * N + s];\n";
            }
            os << "} }\n";
        }
        sync();
        for (std::uint32_t r = 0; r < sv_rounds; ++r) {
            os << "{ const unsigned i = tid + " << r * bs << "u; if (i < " << n_eq << "u) {\n";
            os << "slab[i] = xn" << r << ";\n";
            os << "sjet[" << static_cast<std::uint64_t>(k + 1u) * n_eq << "u + i] = xn" << r << ";\n";
            if (k + 1u == order) {
                os << "mo = hy_max(mo, fabs(xn" << r << "));\n";
            } else if (k + 2u == order) {
                os << "mom1 = hy_max(mom1, fabs(xn" << r << "));\n";
            }
            os << "} }\n";
        }
        sync();
        os << "}\n";
    }
}

// ---- stage 7: the module around the step body ----
void block_gen::module_text()
{
    using emit_detail::prelude;
    using emit_detail::rhofac;

    body = take_os();

    // Scratch per workgroup: tape + state jets.
    const std::uint64_t tape_doubles = static_cast<std::uint64_t>(n_tape) * order * ncp;
    const std::uint64_t sjet_doubles = (static_cast<std::uint64_t>(order) + 1u) * n_eq;
    per_block = (tape_doubles + sjet_doubles + 63u) / 64u * 64u;
    wpb = bs / 64u;

    // Pair phase: the order-0 row of the input jets is recorded together with the state (load / update).
    const std::string ej_rec0
        = on ? "{ const unsigned ee = hy_sv_ej[i]; if (ee != 0xffffu) HY_EJW("
                   + std::to_string(static_cast<std::uint64_t>(order - 1u) * n_ej * 8u) + "u + ee * 8u) = x; } "
             : std::string{};
    src << prelude() << emit_detail::step_loop_source();
    emit_detail::emit_dout(src, p, opts);
    src << tbl.str();
    src << "extern \"C\" __global__ void __launch_bounds__(" << bs << ") hy_taylor(const hy_kargs a)\n{\n";
    // (slab[n_slots]: the slot idle lanes write to; slab[n_slots + 1]: a constant 0.0 - the missing operands of the merged
    // sums of the pair-phase glue.)
    src << "__shared__ double slab[" << n_slots + 2u + (dbuf ? n_eq : 0u) << "];\n";
    if (n_ej != 0u) {
        src << "__shared__ double ejet[" << static_cast<std::uint64_t>(n_ej) * (on ? order : order - 1u) << "];\n";
    }
    src << "__shared__ double red[3 * " << wpb << "];\n__shared__ u64 sh_base;\n__shared__ int sh_nfi;\n";
    src << "const unsigned tid = threadIdx.x;\nconst u64 N = a.N;\n";
    // Per-lane buffer of the updated state values (lane = state variable, strided).
    src << "double c_new[" << sv_rounds << "];\n";
    src << "double *const tape = a.scratch + (u64)blockIdx.x * " << per_block << "ull;\n";
    src << "double *const sjet = tape + " << tape_doubles << "ull;\n";
    src << decl.str();
    src << "if (tid == 0u) slab[" << n_slots + 1u << "] = 0.0;\n";
    src << R"HIP(
for (;;) {
// Pull the next system from the device-side work queue.
__syncthreads();
if (tid == 0u) sh_base = atomicAdd((u64 *)(a.counters + 2), (u64)1);
__syncthreads();
const u64 s = sh_base;
if (s >= N) break;
double t_hi = a.time_hi[s], t_lo = a.time_lo[s];
)HIP";
    for (std::uint32_t i = 0; i < p.n_par; ++i) {
        src << "const double par_" << i << " = a.pars[(u64)" << i << "u * N + s];\n";
    }
    src << "for (unsigned i = tid; i < " << n_eq
        << "u; i += " << bs << "u) { const double x = a.state[(u64)i * N + s]; slab[i] = x; sjet[i] = x; " << ej_rec0
        << "}\n";
    src << R"HIP(
__syncthreads();
HY_STEP_LIMITS(s, HY_DIR_BRANCHY)
HY_STEP_COUNTERS
for (;;) {
HY_STEP_LIM
)HIP";
    src << body;
    // Infinity norms: wave shuffles, then one exchange through LDS.
    for (std::uint32_t m = 1; m < 64u; m *= 2u) {
        src << "m0 = hy_max(m0, __shfl_xor(m0, " << m << ", 64));\n";
        src << "mo = hy_max(mo, __shfl_xor(mo, " << m << ", 64));\n";
        src << "mom1 = hy_max(mom1, __shfl_xor(mom1, " << m << ", 64));\n";
    }
    src << "if ((tid & 63u) == 0u) { red[tid >> 6] = m0; red[" << wpb << "u + (tid >> 6)] = mo; red[" << 2u * wpb
        << "u + (tid >> 6)] = mom1; }\n__syncthreads();\n";
    src << "m0 = red[0]; mo = red[" << wpb << "]; mom1 = red[" << 2u * wpb << "];\n";
    for (std::uint32_t w = 1; w < wpb; ++w) {
        src << "m0 = hy_max(m0, red[" << w << "]); mo = hy_max(mo, red[" << wpb + w << "]); mom1 = hy_max(mom1, red["
            << 2u * wpb + w << "]);\n";
    }
    src << "HY_STEP_SIZE(" << fp_literal(1. / static_cast<double>(order)) << ", " << fp_literal(1. / static_cast<double>(order - 1u))
        << ", " << fp_literal(rhofac(order)) << ")\n";
    // Taylor coefficients on request, then the state update.
    src << "if (a.tc != nullptr) {\nfor (unsigned i = tid; i < " << n_eq << "u; i += " << bs
        << "u) for (unsigned k = 0; k <= " << order << "u; ++k) a.tc[((u64)i * " << (order + 1u)
        << "u + k) * N + s] = sjet[k * " << n_eq << "u + i];\n}\n";
    src << "int nfi = 0;\n";
    // NOTE: the coefficients of a state variable are read back from the per-workgroup array in global memory. As a rolled
    // loop this was ONE load per iteration with a full wait behind it (20 dependent round trips to L2 per state variable and
    // step: ~30 us of a 260 us step on nbody(64)); written out, all the loads of all the rounds of the lane are issued
    // before the first operation - the registers of the order loop are free by now. Branch-free: a lane without a state
    // variable in its last round evaluates a copy of the last variable and the result is ignored.
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        const bool partial = static_cast<std::uint64_t>(r + 1u) * bs > n_eq;
        // (Opaque to the optimiser: as invariants of the step loop the order + 1 addresses of a round are computed once per
        // kernel and spilled - 42 registers reloaded from scratch at every step.)
        src << "unsigned hi" << r << " = " << (partial ? "(tid + " + std::to_string(r * bs) + "u < " + std::to_string(n_eq)
                                                                + "u) ? tid + " + std::to_string(r * bs) + "u : "
                                                                + std::to_string(n_eq - 1u) + "u"
                                                          : "tid + " + std::to_string(r * bs) + "u")
            << ";\nasm volatile(\"\" : \"+v\"(hi" << r << "));\n";
        for (std::uint32_t k = 0; k <= order; ++k) {
            src << "const double hc" << r << "_" << k << " = sjet[" << static_cast<std::uint64_t>(k) * n_eq << "u + hi" << r
                << "];\n";
        }
    }
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        const auto c = [r](std::uint32_t k) { return "hc" + std::to_string(r) + "_" + std::to_string(k); };
        src << "{\n";
        if (opts.high_accuracy) {
            src << "double res = " << c(0) << ", comp = 0.0, cur_h = h;\n";
            for (std::uint32_t k = 1; k <= order; ++k) {
                src << "{\nconst double tmp = " << c(k) << " * cur_h;\nconst double y = tmp - comp;\n";
                src << "const double t = res + y;\ncomp = (t - res) - y;\nres = t;\ncur_h = cur_h * h;\n}\n";
            }
        } else {
            src << "double res = " << c(order) << ";\n";
            for (std::uint32_t k = 1; k <= order; ++k) {
                src << "res = " << c(order - k) << " + res * h;\n";
            }
        }
        src << "if (!hy_finite(res)) nfi = 1;\n";
        // NOTE: sjet row 0 / slab are rewritten only after every lane is done reading the jets.
        src << "c_new[" << r << "] = res;\n}\n";
    }
    src << R"HIP(
HY_STEP_ADVANCE
if (!(hy_finite(t_hi) && hy_finite(t_lo))) nfi = 1;
nfi = __syncthreads_or(nfi);
)HIP";
    src << "for (unsigned i = tid; i < " << n_eq << "u; i += " << bs << "u) { const double x = c_new[i / " << bs
        << "u]; slab[i] = x; sjet[i] = x; " << ej_rec0 << "}\n__syncthreads();\n";
    src << R"HIP(
HY_STEP_TAIL(nfi != 0, tid == 0u)
}
)HIP";
    src << "for (unsigned i = tid; i < " << n_eq << "u; i += " << bs << "u) a.state[(u64)i * N + s] = slab[i];\n";
    src << R"HIP(
if (tid == 0u) {
    HY_STEP_RESULT(s)
}
}
}
)HIP";
}

// ---- stage 8: the emitted module and its notes ----
emitted_module block_gen::result()
{
    emitted_module ret;
    ret.source = src.str();
    ret.kernel_name = "hy_taylor";
    ret.dout_name = "hy_dout";
    ret.block_size = bs;
    ret.lanes_per_system = bs;
    ret.n_clusters = nc;
    ret.lds_bytes = 0;
    ret.mode = emit_mode::block;
    ret.n_statements = e.n_stmt;
    ret.scratch_per_wave = per_block / wpb;
    ret.persistent = true;
    ret.tc_optional = true;
    ret.notes = "block mode: one system per workgroup of " + std::to_string(bs) + " lanes, " + std::to_string(nc)
                + " clusters of " + std::to_string(t0().size()) + " nodes (" + std::to_string(n_tape)
                + " members on the tape, " + std::to_string(n_sto - n_tape) + " recomputed from " + std::to_string(n_ej)
                + " LDS-resident input jets), " + std::to_string(pl.groups.size()) + " glue groups, "
                + std::to_string(n_slots) + " LDS slots, tape " + std::to_string(per_block * 8u / 1024u)
                + " KiB per workgroup";
    // Machine-level loop-invariant code motion off for the pair-phase kernel: invariants of the step loop hoisted in front
    // of it are what the register allocator spills (nbody(64): 54 -> 41 spilled registers, +1.3 %; switch licm: A/B harness).
    if (on && !sw.licm) {
        ret.compile_flags = "-mllvm -disable-machine-licm";
    }
    if (on) {
        ret.block_v2_phase = true;
        ret.notes += "; v2 cluster phase: rolled order loop, " + std::to_string(n_iter) + " rounds per lane, rows < "
                     + std::to_string(M) + " of the tape members in registers, the " + std::to_string(hand)
                     + " most recent rows handed over in registers";
    }
    return ret;
}

} // namespace block_detail

emitted_module emit_block(const taylor_program &p, const emit_options &opts, emit_refusal &why_not)
{
    block_detail::block_gen g(p, opts, why_not);
    if (!g.plan() || !g.input_jets()) {
        return {};
    }
    g.base_tables();
    // (A pair phase which refuses on its parameters has written nothing: the generic cluster phase takes over, on the
    // workgroup size pair_phase_applicable() left.)
    g.on = g.pair_phase_applicable() && g.pair_parameters();
    g.begin_body();
    if (g.on) {
        g.pair_descriptors();
        g.pair_merged_glue();
        g.pair_fused_last_level();
        g.pair_lds_mirrors();
        g.pair_order0();
        g.pair_order_loop();
    } else {
        g.generic_body();
    }
    g.module_text();
    return g.result();
}

} // namespace heyoka_amd
