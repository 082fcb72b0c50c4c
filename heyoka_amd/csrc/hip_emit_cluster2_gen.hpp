// The generator of the pipelined ("v2"), lane-pair ("v3") and one-lane-per-pair ("v5") wave-cluster kernels: one object
// per attempt, its stages in the order the text is produced. Private to hip_emit_cluster2*.cpp:
//   hip_emit_cluster2.cpp         emit_cluster_v2() (retry loop over the lanes per system), the driver run() and the stages
//   hip_emit_cluster2_layout.cpp  the consumer-arranged slab slots of the one-lane-per-pair kernel, table helpers
//   hip_emit_cluster2_orders.cpp  emission helpers, the three order programs, helpers of the module text
// The data the stages share is grouped in the c2_* structs below; a stage reads what the stages before it left there.
#pragma once

#include <array>
#include <map>
#include <set>
#include <tuple>

#include "hip_emit_cluster_plan.hpp"
#include "hip_emit_detail.hpp"

namespace heyoka_amd::cluster2_detail
{

using cluster_detail::cluster_plan;
using cluster_detail::is_var;
using emit_detail::prelude;
using emit_detail::rhofac;
using emit_detail::ssa_emitter;
using psel = ssa_emitter::part_sel;

enum class cluster2_variant { pipelined, lane_pair, one_lane };

// What one attempt of the generator returns: the module (empty source: refused, the reason in why_not) and, typed, what
// emit_cluster_v2() decides its retries on.
struct cluster2_attempt {
    emitted_module mod;
    cluster2_variant variant = cluster2_variant::pipelined;
    bool jets_in_lds = false;
    // The refusal is one which more lanes per system (fewer systems per CU) cure.
    bool more_lanes_cure = false;
};

// ---- Variant: which of the three kernels, and the flags derived from it (computed once). ----
struct c2_variant {
    cluster2_variant variant = cluster2_variant::pipelined;
    bool one_lane = false, pair_split = false;
    bool pairk = false;   // one of the two pair-pattern kernels
    bool m4 = false;      // emit_options::event_stepper
    bool frx = false;     // one lane per pair: reactions fused into the acceleration sums (stage 0c)
    bool fuse_rx = false; // reaction fusion (both pair kernels), see anchors_and_reaction_fusion()
    bool frx_regs = false, merged = false;
    // frx, sums of the later rounds taken from the registers of the first round's lanes by a segmented reduction over
    // adjacent lanes instead of re-read from LDS (plan_lane_sums()).
    bool lane_sum = false;
    // Experiment switches of this generator: ONE environment variable, HEYOKA_AMD_V5_OPTS, a comma-separated list of flags
    // (profiles/experiments/ab.py compares variants inside one process). Every flag switches OFF one of the round-5 items:
    //   nomsq     three accumulators for the half sums of squares (one per coordinate) instead of one;
    //   nopack2   the final evaluation of a partially filled owner slot as a full two-series pass;
    //   notailrd  the jet reads of the final evaluation behind the step size instead of ahead of the selector;
    //   nosc      the selector's logarithm / exponential with literal polynomial constants (hy_sel_log(), exp()).
    //   nolanesum the sums of the rounds after the first read their operands from LDS, one round per L nodes, instead of
    //             adding them across the lanes which hold them (plan_lane_sums()): the text of before that item.
    //   noplainstep every step runs the whole bookkeeping of the step loop (plain_step below): the text of before that item.
    // (nofrx, nobkslab, nowide, novx, nostoreplace, frxlds, norx, bankdbg: where they are read.) Parsed once ('+' separates
    // flags where ',' separates variables: ab.py).
    std::set<std::string> v5_flags;
    bool v5_flag(const char *name) const { return v5_flags.count(name) != 0u; }
    // One lane per pair, jets in LDS, not the stepper with events: a wavefront none of whose systems is finished, clamped,
    // at its step limit or non-finite in this step takes a PLAIN STEP - behind one ballot, only what such a step changes
    // (text_selector(), text_final_evaluation_and_update()). The remaining time is then not carried from step to step: the
    // ordinary path recomputes it from the final time and the current time, and a lower bound of its magnitude (rlb) takes
    // its place in the parked record.
    bool plain_step = false;
};

// ---- Plan and lane geometry. ----
struct c2_geometry {
    cluster_plan pl;
    cluster_detail::pair_pattern pp;
    std::vector<char> cu; // constant_uvars()
    std::uint32_t nc = 0, L = 0, spw = 0, bs = 0, wpb = 0, n_ext = 0, n_out = 0, n_cst = 0;
    const std::vector<std::uint32_t> &t0() const { return pl.clusters[0]; } // the template cluster
    // (The position variables of body sd of the pair of cluster c.)
    std::array<std::uint32_t, 3> body_vars(std::uint32_t c, std::uint32_t sd) const
    {
        return {pl.ext_u[c][pp.de[0][sd]], pl.ext_u[c][pp.de[1][sd]], pl.ext_u[c][pp.de[2][sd]]};
    }
};

// Glue rounds (+ the owner slots of the attached state variables).
struct owner_slot {
    std::size_t out_tbl = 0;  // slab slot of the state variable
    std::size_t var_tbl = 0;  // state-variable index (for the global state array)
    std::uint32_t col = 0;    // owner slot id
    std::uint32_t cbase = 0;  // first jet column of the slot (columns are compressed: one per valid lane)
    std::uint32_t n_valid = 0;
    std::vector<std::string> xname; // SSA names of the coefficients, by order
    bool slab_needed = true;        // is one of the variables of the slot read through the slab?
    // One-lane pair kernel: the second variable of a chain (x' = v) keeps no jet column: its coefficients are
    // re-derived from the column of the first one (parent) in the final evaluation; cbase then counts the
    // order-0 entries of the derived variables (their current values).
    bool derived = false;
    std::uint32_t parent = 0; // owner slot id of the variable it is derived from
    // Lane-reduced sums (lane_sum): lane l owns the jet column utbl[col_tbl][l] (absolute; an idle lane the column of the
    // lane it replicates) and is valid where bit l of valid_mask is set - instead of column cbase + l for l < n_valid.
    // reduced: the slot of a lane-reduced round (its other lanes hold partial sums).
    bool mapped = false, reduced = false;
    std::size_t col_tbl = 0;
    std::uint32_t valid_mask = 0;
};
struct glue_round {
    std::vector<std::size_t> arg_tbl;
    std::size_t out_tbl = 0;
    std::uint32_t n_valid = 0; // lanes l < n_valid own a real node
    bool exported = true;
    std::vector<owner_slot> owners;
    std::vector<std::string> par_name; // per-lane parameter value names, by argument (empty: none)
    std::vector<std::string> c0name;   // names of the constant operands read at order 0, by argument
    std::vector<std::size_t> coef_tbl; // reaction fusion: per-lane coefficient tables, by argument (empty: not fused)
    bool reduced = false;              // lane-reduced round: no operand reads, see emit_glue_compute()
};

// ---- Layout: anchors and owners, slab slots, wide-read / bank-model / bk placement decisions, rounds, jets. ----
struct c2_layout {
    // (att, grp_natt: see anchors_and_reaction_fusion(); grp_natt[g] = attached variables per node of group g.)
    std::map<std::uint32_t, std::vector<std::uint32_t>> att;
    std::vector<std::uint32_t> grp_natt;
    std::vector<char> rx_fused;
    std::vector<std::uint32_t> rx_src;
    std::vector<char> glue_read;
    std::vector<std::uint32_t> lane_pr, lane_rx; // one-lane pair kernel: output slot triples of the lanes
    bool wide_rd = false;                        // ... wide-read layout: slots arranged by consumer (see below)
    // ... velocity exchange: the pair lanes take the coordinate differences from the velocity jets, d^[k] = (v_a^[k-1] - v_b^[k-1])
    // RN(1 / k), and no position coefficient is published (see below). vx_col[l] = first jet column of the two bodies of lane l.
    bool vexch = false;
    std::vector<std::array<std::uint32_t, 2>> vx_col;
    std::vector<std::array<std::uint32_t, 3>> wide_pr, wide_rx; // ... its output slots, per lane and coordinate
    std::uint32_t slab_stride_opt = 0;
    std::uint64_t bank_cost = 0;
    bool bk_in_slab = false;
    // The analysis behind the wide-read layout (layout_one_lane()).
    std::vector<std::array<std::uint32_t, 3>> bodies; // position variables (x, y, z) of every body
    std::vector<std::uint32_t> node_coord, node_rank;   // per node of the glue group
    std::uint32_t n_rank = 0, n_args = 0;
    // Lane-reduced sums (lane_sum, plan_lane_sums()): index in the sum group of the node which lane l computes in the first
    // round (ls_first) and receives from the reduction (ls_last; ~0u: none), and the operand position of the first-round
    // sums whose register holds the terms; ls_park: the first-round node on whose jet column a lane without a later sum parks
    // its store of the reduced round.
    std::vector<std::uint32_t> ls_first, ls_last, ls_park;
    std::uint32_t ls_pos = 0;
    // LDS layout (doubles): buf_stride between the two parity buffers, slab_stride per system.
    std::uint32_t dummy_base = 0, n_slots_tot = 0, buf_stride = 0, slab_stride = 0;
    std::vector<std::vector<glue_round>> rounds;
    std::uint32_t n_own = 0;
    // Columns of the state-variable jets: one per state variable (owner slots are compressed: only the valid lanes
    // of a slot own a column) plus one dummy column per system which absorbs the stores of the idle lanes of a
    // partially filled slot - they replicate the node of a valid lane, so every statement of the step body is
    // unconditional (no exec-mask manipulation inside the step loop).
    std::uint32_t n_col = 0;
    // (One-lane pair kernel: no dummy column - the idle lanes of a partially filled slot store to the entry they
    // replicate - and a row is laid out [owner slot][system][lane]: the 32 lanes which a ds_read_b64 services together
    // (two systems) then touch 32 consecutive doubles, i.e. every bank once.)
    std::uint32_t n_colp = 0;
    // (One-lane pair kernel: current values of the derived variables, [system of the wave][entry] + one dummy entry.)
    std::uint32_t n_dcol = 0, n_dcolp = 0;
    std::uint32_t n_hslots = 0; // lane slots of the final Horner / compensated evaluation
    std::uint64_t jet_rows_doubles = 0, jet_doubles_per_wave = 0;
    bool jet_lds = false, compact_tc = false;
    std::size_t n_tc_rows = 0; // rows of the mode-4 store (tables_of_the_jet_placement())
};

// ---- Tables: per-lane unsigned / double tables (indices handed out in insertion order) and who owns which. ----
struct c2_tables {
    std::vector<std::vector<std::uint32_t>> utbl;
    std::vector<std::vector<double>> dtbl;
    // NOTE: tables of slab slots and tables of state-variable indices are kept apart (the slot tables are
    // renumbered by the bank-conflict optimiser below).
    std::vector<char> utbl_is_slot;
    // utexpr[t]: how the kernel refers to the per-lane value of table t - a register loaded at the top of the kernel
    // ("ut<t>"), or (one-lane pair kernel, where every register counts) an earlier table plus a constant when the two
    // differ by the same amount on every lane (the three coordinates of a body, the three products of a pair: the
    // constant folds into the offset field of the LDS instruction).
    std::vector<std::string> utexpr;
    // Lane-pair variant: lane l = 2 * pair + role (role 0 = A: d_0, d_1; role 1 = B: d_2 and the pow); the lanes
    // beyond the last pair replicate pair 0 and write to dummy slots.
    struct pair_tables {
        std::size_t s0 = 0, s1 = 0, p0 = 0, p1 = 0, os = 0, op = 0, rs = 0, rp = 0, csc = 0, crs = 0, crp = 0;
    } pt;
    // One-lane pair kernel: lane l = pair l (the lanes beyond the last pair replicate pair 0 and write to dummy slots).
    struct single_tables {
        std::size_t s[3][2] = {}, o[3] = {}, r[3] = {}, csc = 0, crs = 0;
    } st1;
    std::vector<std::size_t> ext_tbl, out_tbl, cst_tbl;
    // Per-lane parameters: tables of parameter indices; the values are loaded when a group of systems is picked up.
    std::vector<std::size_t> lane_par_tbls;
    std::map<std::uint32_t, std::array<std::size_t, 3>> pk_tbl; // packed final evaluation, see pack_tail_slot()
};

// The passes of the final evaluation of the one-lane kernel, in order: one per variable with a jet column (ow), with the
// variable derived from it (dv: x' = v, at most one - chains of length <= 2); `packed` = the partially filled owner
// slot which runs one series per lane. rows / facs: the names of the jet rows (and of the factors RN(1 / k) of a packed
// pass) where their LDS reads have been issued ahead of the selector - empty otherwise.
struct tail_pass {
    const owner_slot *ow, *dv;
    bool packed;
    std::vector<std::string> rows, facs;
};

// ---- SSA emitter, output streams, and the state of the order programs and of the module text. ----
struct c2_emit {
    c2_emit(const taylor_program &p, std::uint32_t order) : e(p, order), os(e.os) {}
    ssa_emitter e;
    std::ostringstream &os; // the step body, through the SSA emitter
    std::ostringstream src; // the module
    std::string body;
    std::uint32_t n_wide = 0;
    // NOTE: the history chains of order k can be emitted in several parts: the first one at the end of
    // order k - 1 (it overlaps the glue exchange), the others at the beginning of the cluster phase of
    // order k. Measured on gfx950 (outer-SS, 1 048 576 systems): 18.11 ms per launch for 1, 2 and 3 parts
    // - the chains only touch registers, so the compiler's scheduler already moves them across the
    // compiler-only HY_WSYNC barrier. Hence the default of a single part.
    static constexpr std::uint32_t n_parts = 1;
    std::vector<std::uint32_t> t0_ids;
    // Explicit overlap of the LDS exchange latency (the workgroup runs one wavefront per SIMD, nobody else
    // hides it): in both exchange regions of an order the LDS reads are issued first, then - fenced by
    // scheduling barriers - a chunk of history-chain FMAs which do not depend on them, then the dependent
    // computation. The chunks are (ssa_emitter::emit_partials_sel): in the cluster region of order k the second
    // half of the early terms of order k + 1; in the last glue region of order k the late terms of order k + 1
    // and the first half of the early terms of order k + 2.
    static constexpr bool overlap = true, fence2 = true;
    // Lane-pair program (see emit_pair_compute()).
    std::vector<std::string> aP, aR, aRp, aS;
    std::string hc1, hc2, hc3, hc4, hmid;
    bool has_rx = false, pow_norm = false;
    std::string rb1, ap0x2; // 1 / b_0 (lane B), 2 aP[0]
    // One-lane pair program (see emit_single_compute()).
    std::vector<std::string> sD[3], sB, sA;
    std::string hq[3], hm[3], hcx[3], hT, hU, pow_pre;
    unsigned pad_chain = 0, pad_dep = 0, pad_st = 0, pad_ld = 0, pad_salu = 0, pad_regs = 0;
    bool any_pad = false, exp_norx = false, merged_sq = false, sel_scalar = false, prio_switch = false;
    int prio_mode = 0;
    std::vector<char> ext_const;
    // Module text: the event equations inside the stepper, the bookkeeping block, the tail of the step.
    bool ev_inline = false;
    // (lane -> (event, constant) of the close-encounter events which the lane of a pair contributes itself.)
    std::map<std::uint32_t, std::pair<std::uint32_t, double>> pe_lane_ev;
    std::map<std::uint32_t, double> pe_lane_sign; // (-1: the event equation is c - |r_i - r_j|^2)
    std::string ev_code;
    std::vector<std::vector<std::string>> ev_coeffs;
    std::vector<std::string> pe_g;
    bool bk_lds = false;
    static constexpr const char *bk_fields_d[] = {"t_hi", "t_lo", "tfin.hi", "tfin.lo", "rem.hi", "rem.lo", "mdt", "step_lim", "min_h", "max_h", "last_h", "thr"};
    std::vector<tail_pass> tail_passes;
    std::uint64_t kstride = 0; // (Doubles between two rows of a jet column.)
    std::uint32_t n_trd = 0, n_trd_used = 0;
};

struct cluster2_gen : c2_variant, c2_geometry, c2_layout, c2_tables, c2_emit {
    const taylor_program &p;
    const emit_options &opts;
    emit_refusal &why_not;
    const bool allow_one_lane;
    // (min_lanes: the smallest number of lanes per system of the one-lane-per-pair kernel - see emit_cluster_v2().)
    const std::uint32_t min_lanes, n_eq, order;
    cluster2_attempt res;

    cluster2_gen(const taylor_program &p, const emit_options &opts, emit_refusal &why_not, bool allow_one_lane, std::uint32_t min_lanes);
    cluster2_attempt run();

    // Stages, in the order run() calls them (the stage table of hip_emit_cluster2.cpp); a stage which refuses sets why_not.
    void plan_and_select_variant(), anchors_and_reaction_fusion(), layout_one_lane(), lds_layout_and_lane_tables(),
        build_glue_rounds(), layout_jets_and_schedule(), init_order_programs(), emit_step_body(),
        text_helpers_and_constant_tables(), text_kernel_prologue(), text_event_equations(), text_pickup(), text_selector(),
        text_event_exclusion(), text_final_evaluation_and_update(), text_refill_and_tail(), finish();
    // Parts of layout_jets_and_schedule(): the LDS budget. lds_limit_bytes: the LDS of a CU, what a workgroup may declare.
    static constexpr std::uint64_t lds_limit_bytes = 160u * 1024u;
    struct lds_array {
        const char *name;
        std::uint32_t elem_bytes;
        std::uint64_t count;
    };
    void tables_of_the_jet_placement();
    std::vector<lds_array> lds_arrays() const;
    std::uint64_t lds_footprint() const, lds_count(const char *name) const;
    // Parts of plan_and_select_variant() and of layout_one_lane().
    void number_glue_slots(std::uint32_t ns), place_wide_read_slots(), plan_lane_sums(std::uint32_t n_first), renumber_sv_slots();
    // The rounds of a glue group and the node (index in the group) which lane l computes in round r; false: the lane has
    // no node of its own there and replicates that one. (One round per L nodes in order, unless lane_sum arranges them.)
    std::uint32_t n_rounds_of(std::size_t g) const;
    std::pair<std::uint32_t, bool> round_node(std::size_t g, std::uint32_t r, std::uint32_t l) const;
    template <typename F>
    void for_each_owner(F &&f) // f(glue round, owner slot), in the order of the rounds
    {
        for (auto &rg : rounds) {
            for (auto &gr : rg) {
                for (auto &ow : gr.owners) {
                    f(gr, ow);
                }
            }
        }
    }

    // Tables and their names.
    std::size_t add_utbl(std::vector<std::uint32_t> v, bool is_slot = true);
    std::size_t add_dtbl(std::vector<double> v);
    std::string utname(std::size_t t) const { return utexpr[t]; }
    // (One-lane pair kernel: the per-lane constants live in LDS and are read where they are used - one address register
    // for all of them instead of two registers each.)
    std::string dtname(std::size_t t) const { return one_lane ? ("dtl[" + std::to_string(t * L) + "]") : ("dt" + std::to_string(t)); }
    std::string coefname(std::size_t t) const { return frx_regs ? ("frc" + std::to_string(t)) : dtname(t); }
    std::uint32_t pr_slot(std::uint32_t pr_u, std::uint32_t rx_u, std::uint32_t dflt) const;
    std::string lane_par(std::vector<std::uint32_t> idx);
    // Position of an owner slot inside a row of the jets (one-lane pair kernel): rows are [owner slot][system][lane] - the 32
    // lanes which a ds_read_b64 services together touch 32 consecutive doubles - or, with the velocity exchange,
    // [system][column] - the three coordinates of a body adjacent. jet_off: first entry of the slot for the first system
    // of the wavefront, jet_sys: distance between two systems.
    std::uint64_t jet_off(const owner_slot &ow) const { return vexch ? ow.cbase : static_cast<std::uint64_t>(spw) * ow.cbase; }
    std::uint32_t jet_sys(const owner_slot &ow) const { return vexch ? (ow.derived ? n_dcol : n_col) : ow.n_valid; }
    bool pack_tail_slot(const owner_slot &ow, const owner_slot *dv) const;
    // Emission helpers (stage 4) and the order programs.
    std::string slabk(std::uint32_t k, const std::string &tbl) const;
    std::string jet_at(std::uint32_t k, std::uint32_t col) const
    {
        return "jc" + std::to_string(col) + "[" + std::to_string(static_cast<std::uint64_t>(k) * spw * n_colp) + "]";
    }
    void sync() { os << "HY_WSYNC();\n"; }
    void sched_fence() { os << "__builtin_amdgcn_sched_barrier(0);\n"; }
    // Where the current value (order 0) of the variables of an owner slot lives: read side (the idle lanes of a partially
    // filled slot read the entry of a valid lane) and write side (... and write to the dummy entry).
    std::string row0_r(const owner_slot &ow) const { return (ow.derived ? "x0r" : "jr") + std::to_string(ow.col) + "[0]"; }
    std::string row0_w(const owner_slot &ow) const { return (ow.derived ? "x0c" : "jc") + std::to_string(ow.col) + "[0]"; }
    void publish_sv(owner_slot &ow, std::uint32_t k, const std::string &name);
    std::string wide_read(const std::string &tbl);
    std::vector<std::string> emit_glue_reads(std::size_t g, std::uint32_t r, std::uint32_t k), emit_pair_reads(std::uint32_t k),
        emit_single_reads(std::uint32_t k);
    void emit_glue_compute(std::size_t g, std::uint32_t r, std::uint32_t k, const std::vector<std::string> &names),
        emit_pair_compute(std::uint32_t k, const std::vector<std::string> &rdv);
    void emit_glue_round(std::size_t g, std::uint32_t r, std::uint32_t k) { emit_glue_compute(g, r, k, emit_glue_reads(g, r, k)); }
    void emit_pair_order(std::uint32_t k) { emit_pair_compute(k, emit_pair_reads(k)); }
    // (Tried in round 5 and removed: the stores of a round spread over the convolution chains which follow it instead of a
    // burst at the end of the dependent section - the eight wavefronts of a CU queue on one LDS store path -: -1.6 %,
    // profiles/r05_ab_spread_stores.log; the early chain terms of order k + 1 interleaved with the dependent operations of
    // round k: -1 %, profiles/r05_ab_interleaved_early_terms.log.)
    void emit_store(const std::string &stmt) { os << stmt; }
    void emit_single_compute(std::uint32_t k, const std::vector<std::string> &rdv), emit_single_history(std::uint32_t k), emit_cluster(std::uint32_t k);
    // Module text helpers.
    void bk_store(int which = 0), bk_load();
    std::string bk_field(const char *nm) const;
    std::string tail_val(const std::vector<std::string> &names, std::uint32_t k, const std::string &ex);
};

} // namespace heyoka_amd::cluster2_detail
