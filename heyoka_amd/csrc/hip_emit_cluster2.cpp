// Cluster code generation, version 2: software-pipelined orders.
//
// Same partition as hip_emit_cluster.cpp (clusters in registers, glue through an LDS slab), with the
// per-order critical path shortened:
//   * state-variable recursions are *fused* into the glue round that produces their right-hand side
//     (x^[k+1] = rhs^[k] / (k + 1) is computed by the lane that just computed rhs^[k]; chains such as
//     x' = v, v' = a ride along), so that an order needs one LDS synchronisation per dependency level
//     (2 for N-body systems) instead of two extra ones for a separate state-variable phase;
//   * the LDS slab is double-buffered by order parity (no write-after-read hazards between orders);
//   * the history part of every convolution of order k + 1 (terms without order-(k+1) operands) is
//     emitted at the end of order k, where it overlaps the latency of the glue exchange; only the
//     1-2 terms involving new coefficients remain on the critical path (ssa_emitter::node_partial /
//     node_finish). Sums are FMA chains;
//   * divisions by the (constant) order use the exact FMA-based sequence ssa_emitter::div_const().
// The generator is the object cluster2_gen (hip_emit_cluster2_gen.hpp); this file holds its driver, the selection of the
// variant and emit_cluster_v2(), the retry loop over the lanes per system.
#include <algorithm>
#include <cstdio>
#include <functional>

#include "hip_emit_cluster2_gen.hpp"
#include "logging.hpp"

namespace heyoka_amd::cluster2_detail
{

cluster2_gen::cluster2_gen(const taylor_program &p_, const emit_options &opts_, emit_refusal &why_not_, bool allow_one_lane_,
                           std::uint32_t min_lanes_)
    : c2_emit(p_, opts_.order), p(p_), opts(opts_), why_not(why_not_), allow_one_lane(allow_one_lane_), min_lanes(min_lanes_),
      n_eq(p_.n_eq), order(opts_.order)
{
    std::string s = opts.dev.v5_opts;
    std::replace(s.begin(), s.end(), '+', ',');
    for (std::size_t b = 0, en = 0; b <= s.size(); b = en + 1u) {
        en = std::min(s.find(',', b), s.size());
        v5_flags.insert(s.substr(b, en - b));
    }
}

// The stages in the order the text is produced; a stage which refuses leaves the reason in why_not (empty until then:
// the first stage assigns it) and the module empty.
cluster2_attempt cluster2_gen::run()
{
    static constexpr void (cluster2_gen::*const stages[])() = {
        &cluster2_gen::plan_and_select_variant, &cluster2_gen::anchors_and_reaction_fusion, &cluster2_gen::layout_one_lane,
        &cluster2_gen::lds_layout_and_lane_tables, &cluster2_gen::build_glue_rounds, &cluster2_gen::layout_jets_and_schedule,
        &cluster2_gen::init_order_programs, &cluster2_gen::emit_step_body,
        &cluster2_gen::text_helpers_and_constant_tables, &cluster2_gen::text_kernel_prologue, &cluster2_gen::text_event_equations,
        &cluster2_gen::text_pickup, &cluster2_gen::text_selector, &cluster2_gen::text_event_exclusion,
        &cluster2_gen::text_final_evaluation_and_update, &cluster2_gen::text_refill_and_tail, &cluster2_gen::finish};
    for (const auto stage : stages) {
        (this->*stage)();
        if (!why_not.empty()) {
            break;
        }
    }
    return std::move(res);
}

// The glue nodes are numbered after the cluster outputs (both pair kernels).
void cluster2_gen::number_glue_slots(std::uint32_t ns)
{
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (pl.cluster_of[u] == -1) {
            pl.slot_of[u] = static_cast<int>(ns++);
        }
    }
    pl.n_slots = ns;
}

// Stages 0 / 0b / 0c: the plan (cluster_detail::make_plan(), pair pattern), which of the three kernels serves it, the lanes
// per system, the slab slots of the cluster outputs in lane order, the reactions fused into the sums. Reads p, opts,
// allow_one_lane, min_lanes; leaves pl, pp, cu, the variant flags, the lane geometry (L, spw, bs, wpb, n_ext, n_out, n_cst)
// and frx (with the nodes of the sum group reordered).
void cluster2_gen::plan_and_select_variant()
{
    // Parameter operands are per-lane values here (e.g. kw::masses = par[...]: the pair clusters differ only by the
    // indices of the parameters they read).
    cluster_detail::plan_limits plim;
    plim.generic_pars = true;
    why_not = cluster_detail::make_plan(p, opts.order, pl, plim);
    if (!why_not.empty()) {
        return;
    }
    cu = constant_uvars(p);
    nc = static_cast<std::uint32_t>(pl.clusters.size());

    // ---- 0. Lane-pair variant ("v3"): point-mass pair clusters {d_0, d_1, d_2 = coordinate differences,
    // sum_sq(d_0, d_1, d_2), pow(sum_sq, alpha), [c * pow], d_i * pow, [c_i * (d_i * pow)]} are split over TWO lanes:
    // lane A owns d_0, d_1 (their products and squares), lane B owns d_2, the sum of squares and the pow recurrence.
    // Each lane keeps 4 coefficient histories instead of 5 + and the kernel fits in 256 registers, i.e. two wavefronts
    // per SIMD: with one wavefront per SIMD every instruction of the stream - LDS, scalar, register copies - costs an
    // issue slot of the FP64 pipe (profiles/ubench/issue_rate.hip), with two they overlap with the other wavefront's
    // arithmetic. The two lanes run ONE instruction stream: the chains are matched so that the same FMA is useful
    // work on both lanes with different register contents (see emit_pair_order below).
    cluster_detail::detect_pair_pattern(p, pl, pp);
    const bool pp_shape_ok = pp.ok;
    {
        const bool ok = pp.ok;
        // NOTE: up to 32 pairs. With 17 .. 32 pairs there is one system per wavefront (64 lanes per system); in round 2
        // that variant did not terminate on the hardware: a finished system kept taking steps whose length was only
        // clamped to zero (a nan from the selector of a non-finite state survives the clamp), fixed by forcing h = 0.
        pp.ok = ok && 2u * nc <= 64u && p.n_par == 0u && (opts.cluster_kernel == 0 || opts.cluster_kernel >= 3);
    }
    m4 = opts.event_stepper;
    // ---- 0b. One lane per pair, two wavefronts per SIMD ("v5"): the lane-pair split halves the histories a lane keeps
    // (4 x 20 doubles) so that the kernel fits in 256 registers, but every piece of work outside the convolution
    // chains - the role union of the finishing operations, the glue round, the serial tail of the step - is then paid
    // per TWO systems of a wavefront. Five histories (d_0, d_1, d_2, b / b_0, sa) of 19 entries fit in 256 registers as
    // well once the pow recurrence stops keeping j * sa_j: with T_j = sum_{i >= j} p_i (p_i = b_{k-i} sa_i) the weighted
    // sum is a sum of suffix sums, S2 = sum_j j p_j = sum_j T_j - one FMA and one addition per term, like the two FMAs
    // of the weighted form, and no sixth history. One lane per pair: 16 lanes per system for the 15 pairs of the outer
    // Solar System, FOUR systems per wavefront, no role union and no lane exchanges inside a pair. The jets of the
    // state variables of 32 systems per CU do not fit in LDS (199 KB): only the velocity-type variables (the ones
    // defined by a glue node) are stored, the coefficients of the position-type ones (x' = v) are re-derived in the final
    // evaluation as x^[k] = v^[k-1] * RN(1 / k) - the very operation which produced them.
    one_lane = [&]() {
        if (!allow_one_lane) {
            return false;
        }
        // (The derived position jets rely on the reciprocal form of the division by the order.)
        // (Stepper with events: this kernel keeps exactly the COMPACT set of Taylor coefficients - velocity-type jets and
        // the current values of the position-type variables -, see emitted_module::compact_tc; HEYOKA_AMD_V5_EVENTS=0 and
        // HEYOKA_AMD_COMPACT_TC=0 keep the stepper with events on the lane-pair kernel.)
        const bool m4_ok = !m4 || (opts.dev.v5_events && opts.dev.compact_tc);
        return pp_shape_ok && p.n_par == 0u && m4_ok && nc <= 64u && !opts.exact_division;
    }();
    if (one_lane) {
        pp.ok = false;
    }
    pair_split = pp.ok;
    // (Shared by the two pair-pattern kernels: fused reactions, merged schedule, reciprocal-based divisions.)
    pairk = pair_split || one_lane;
    if (pair_split) {
        pl.L = 2;
        while (pl.L < 2u * nc) {
            pl.L *= 2u;
        }
        pl.spw = 64u / pl.L;
        // Slab slots of the cluster outputs in lane order: the lanes of a group write consecutive doubles (distinct LDS
        // banks). d_0 * sa / d_2 * sa alternate (lane = 2 * pair + role), d_1 * sa is written by the A lanes only.
        std::uint32_t ns = n_eq;
        std::fill(pl.slot_of.begin() + n_eq, pl.slot_of.end(), -1);
        const auto number = [&](const auto &member_of_lane, std::uint32_t n_lanes) {
            for (std::uint32_t l = 0; l < n_lanes; ++l) {
                pl.slot_of[member_of_lane(l)] = static_cast<int>(ns++);
            }
        };
        number([&](std::uint32_t l) { return pl.clusters[l / 2u][pp.pr[(l & 1u) != 0u ? 2u : 0u]]; }, 2u * nc);
        number([&](std::uint32_t c) { return pl.clusters[c][pp.pr[1]]; }, nc);
        if (pp.rx[0] >= 0) {
            number([&](std::uint32_t l) {
                return pl.clusters[l / 2u][static_cast<std::uint32_t>(pp.rx[(l & 1u) != 0u ? 2u : 0u])];
            }, 2u * nc);
            number([&](std::uint32_t c) { return pl.clusters[c][static_cast<std::uint32_t>(pp.rx[1])]; }, nc);
        }
        number_glue_slots(ns);
    }
    if (one_lane) {
        pl.L = min_lanes;
        while (pl.L < nc) {
            pl.L *= 2u;
        }
        pl.spw = 64u / pl.L;
        // Outputs in lane order, one run of consecutive slots per product.
        std::uint32_t ns = n_eq;
        std::fill(pl.slot_of.begin() + n_eq, pl.slot_of.end(), -1);
        // (Numbered again after the compaction below: [lane][product] with a stride of 3 doubles between the lanes of a
        // group - the 16 lanes which a ds_write_b64 services together hit 16 different bank pairs -, the reactions in a
        // second region of the same shape.)
        for (std::uint32_t c = 0; c < nc; ++c) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                pl.slot_of[pl.clusters[c][pp.pr[i]]] = static_cast<int>(ns++);
            }
        }
        for (std::uint32_t c = 0; pp.rx[0] >= 0 && c < nc; ++c) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                pl.slot_of[pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])]] = static_cast<int>(ns++);
            }
        }
        number_glue_slots(ns);
    }
    L = pl.L, spw = pl.spw;
    // (Lane pairs / one lane per pair: 512 threads = two wavefronts per SIMD.)
    bs = pairk ? 512u : 256u;
    wpb = bs / 64u;
    n_ext = static_cast<std::uint32_t>(pl.ext_u[0].size());
    n_out = static_cast<std::uint32_t>(pl.out_pos.size());
    n_cst = static_cast<std::uint32_t>(pl.cst_pos.size());

    variant = one_lane ? cluster2_variant::one_lane : (pair_split ? cluster2_variant::lane_pair : cluster2_variant::pipelined);
    // ---- 0c. One lane per pair: reactions fused into the acceleration sums ("frx", round 5). The sensitivity experiment
    // (profiles/r05_sensitivity_marginal_costs.log) prices an LDS store at ~30 cycles of the issuing wavefront's time, five
    // FMAs; 3 of the 8 stores of an order are the reactions c * (d_i * sa), values which differ from the direct products
    // by a per-pair factor. Dropping them (timing experiment "norx", profiles/r05_ab_fused_reactions_estimate.log) is worth
    // +7.8 %. Here the sums of the first glue round read the direct product wherever they read a reaction and apply the
    // factor themselves, t_a = c_a * p_a with per-lane coefficients (c, or 1.0 for a direct product: exact, so that without
    // FMA contraction every term is rounded like the separate node); the additions keep the reference's pairwise order.
    // Registers are what this costs (five coefficient doubles per lane through the orders), so the coefficients exist only
    // once: the nodes of the sum group are reordered so that the sums made of direct products alone (the first body of every
    // pair it takes part in) come last - the rounds after the first are then plain sums without coefficients.
    frx = false;
    lane_sum = false;
    if (one_lane && !m4 && pp.rx[0] >= 0 && pl.groups.size() == 1u && !v5_flag("nofrx")) {
        auto &nodes = pl.groups[0].nodes;
        std::map<std::uint32_t, bool> is_rx_out; // cluster output -> is it a reaction?
        for (std::uint32_t c = 0; c < nc; ++c) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                is_rx_out[pl.clusters[c][pp.pr[i]]] = false;
                is_rx_out[pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])]] = true;
            }
        }
        const auto &n0 = p.nodes[nodes[0] - n_eq];
        frx = n0.kind == func_kind::sum && n0.args.size() >= 2u;
        std::vector<char> plain(nodes.size(), 1);
        for (std::size_t j = 0; j < nodes.size() && frx; ++j) {
            const auto &nd = p.nodes[nodes[j] - n_eq];
            frx = nd.kind == func_kind::sum && nd.args.size() == n0.args.size();
            for (const auto &o : nd.args) {
                const auto it = is_var(o) ? is_rx_out.find(o.idx) : is_rx_out.end();
                frx = frx && it != is_rx_out.end();
                if (frx && it->second) {
                    plain[j] = 0;
                }
            }
        }
        if (frx) {
            // (Stable: the three coordinates of a body stay adjacent and in order, which the velocity exchange relies on.)
            std::vector<std::uint32_t> first, last;
            for (std::size_t j = 0; j < nodes.size(); ++j) {
                (plain[j] != 0 ? last : first).push_back(nodes[j]);
            }
            // Every round after the first must consist of plain sums.
            frx = first.size() <= pl.L && !last.empty();
            if (frx) {
                const auto n_first = static_cast<std::uint32_t>(first.size());
                first.insert(first.end(), last.begin(), last.end());
                nodes = std::move(first);
                // (The plain sums by a reduction over the lanes of the first round where the plan allows it.)
                if (!v5_flag("nolanesum")) {
                    plan_lane_sums(n_first);
                }
            }
        }
    }
}

// Renumber the slab slots of the state variables in owner order (group, round, chain position, lane), so
// that the lanes publishing new coefficients write consecutive slots (distinct LDS banks).
void cluster2_gen::renumber_sv_slots()
{
    std::uint32_t next = 0;
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &nodes = pl.groups[g].nodes;
        for (std::uint32_t r = 0; r < n_rounds_of(g); ++r) {
            for (std::uint32_t a = 0; a < grp_natt[g]; ++a) {
                for (std::uint32_t l = 0; l < L; ++l) {
                    if (const auto [j, valid] = round_node(g, r, l); valid) {
                        pl.slot_of[att.at(nodes[j])[a]] = static_cast<int>(next++);
                    }
                }
            }
        }
    }
    if (next != n_eq) {
        why_not = "internal error: state-variable slots";
    }
}

// Stage 1, first part. Reads the plan, the pair pattern and frx; leaves att, grp_natt, the slab slots of the state variables
// renumbered in owner order, rx_fused, rx_src, fuse_rx, frx (final) and glue_read.
void cluster2_gen::anchors_and_reaction_fusion()
{
    // ---- 1. Anchor every state variable to the glue node at the root of its rhs chain. ----
    // anchor[i] = glue u variable, depth[i] >= 1.
    std::vector<int> anchor(n_eq, -1);
    std::vector<std::uint32_t> depth(n_eq, 0);
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        std::uint32_t cur = i, d = 0;
        std::set<std::uint32_t> seen;
        for (;;) {
            if (!seen.insert(cur).second) {
                why_not = "cyclic chain of state-variable definitions";
                return;
            }
            const auto &def = p.sv_defs[cur];
            ++d;
            if (def.type != operand::kind::uvar) {
                why_not = "a state variable is defined by a constant or a parameter";
                return;
            }
            if (def.idx < n_eq) {
                cur = def.idx;
                continue;
            }
            if (pl.cluster_of[def.idx] != -1) {
                why_not = "a state variable is defined directly by a cluster member";
                return;
            }
            anchor[i] = static_cast<int>(def.idx);
            depth[i] = d;
            break;
        }
    }
    // att[u] = state variables anchored at glue node u, sorted by depth.
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        att[static_cast<std::uint32_t>(anchor[i])].push_back(i);
    }
    for (auto &[u, v] : att) {
        std::sort(v.begin(), v.end(), [&](std::uint32_t a, std::uint32_t b) { return depth[a] < depth[b]; });
        for (std::size_t j = 0; j < v.size(); ++j) {
            // Chain shape: depths 1, 2, 3, ... each defined by the previous one (or by the anchor).
            if (depth[v[j]] != j + 1u) {
                why_not = "branching state-variable chains";
                return;
            }
            const auto &def = p.sv_defs[v[j]];
            const auto expect = (j == 0u) ? u : v[j - 1u];
            if (def.idx != expect) {
                why_not = "branching state-variable chains";
                return;
            }
        }
    }
    // All the nodes of a glue group must carry the same number of attached variables.
    grp_natt.assign(pl.groups.size(), 0);
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &nodes = pl.groups[g].nodes;
        const auto it0 = att.find(nodes[0]);
        const auto n0 = it0 == att.end() ? 0u : static_cast<std::uint32_t>(it0->second.size());
        for (const auto u : nodes) {
            const auto it = att.find(u);
            const auto n = it == att.end() ? 0u : static_cast<std::uint32_t>(it->second.size());
            if (n != n0) {
                why_not = "glue nodes of one group with different state-variable chains";
                return;
            }
        }
        grp_natt[g] = n0;
    }

    renumber_sv_slots();
    if (!why_not.empty()) {
        return;
    }

    // Reaction fusion (lane-pair variant): the members c * pr of a cluster (the reaction on the second body of the pair)
    // are not computed / exported by the cluster lanes: the glue sums which read them read the direct product pr instead
    // and multiply it by a per-lane coefficient (c, or 1.0 where the sum reads the direct product itself: exact, so the
    // rounding sequence of every term is the one of the separate node). Two LDS stores less per order and lane.
    // rx_fused[u] = 1 for the fused members; rx_src[u] = the product they scale.
    rx_fused.assign(p.n_u, 0);
    rx_src.assign(p.n_u, 0);
    fuse_rx = false;
    if (pairk && pp.rx[0] >= 0) {
        // (One-lane pair kernel: the reactions are computed and exported by the pair lane - the slab of a system is
        // single-buffered there and has room for them - so that the sums need no per-lane coefficients: 20 registers.)
        fuse_rx = !one_lane || frx;
        for (std::size_t c = 0; c < nc; ++c) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                const auto u = pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])];
                rx_fused[u] = 1;
                rx_src[u] = pl.clusters[c][pp.pr[i]];
            }
        }
        std::vector<char> in_sum_group(p.n_u, 0);
        for (const auto &g : pl.groups) {
            const auto &n0 = p.nodes[g.nodes[0] - n_eq];
            const bool all_var = std::all_of(n0.args.begin(), n0.args.end(), [](const operand &o) { return is_var(o); });
            if (n0.kind == func_kind::sum && all_var) {
                for (const auto u : g.nodes) {
                    in_sum_group[u] = 1;
                }
            }
        }
        for (std::uint32_t u = n_eq; fuse_rx && u < p.n_u; ++u) {
            for (const auto &o : p.nodes[u - n_eq].args) {
                if (is_var(o) && rx_fused[o.idx] != 0 && in_sum_group[u] == 0) {
                    fuse_rx = false;
                }
            }
        }
        for (const auto &d : p.sv_defs) {
            if (is_var(d) && rx_fused[d.idx] != 0) {
                fuse_rx = false;
            }
        }
        if (!fuse_rx) {
            std::fill(rx_fused.begin(), rx_fused.end(), 0);
        }
    }
    frx = frx && fuse_rx;
    if (lane_sum && !frx) {
        // (Without the fused reactions: the rounds, and the slots numbered after them above, as they were.)
        lane_sum = false;
        renumber_sv_slots();
        if (!why_not.empty()) {
            return;
        }
    }
    // A glue node / state variable needs a slab slot only if somebody reads it through the slab.
    glue_read.assign(p.n_u, 0);
    for (const auto &n : p.nodes) {
        for (const auto &o : n.args) {
            if (is_var(o)) {
                glue_read[o.idx] = 1;
            }
        }
    }
}

// Stage 1, one-lane pair kernel only: the slab of a system. Reads glue_read, the fusion flags and the stages before it;
// leaves bk_in_slab, wide_rd, vexch, vx_col, the slab compacted to the slots which are read through it, the lane permutations
// lane_pr / lane_rx (or wide_pr / wide_rx), slab_stride_opt and bank_cost of the bank-model search, pl.slot_of, pl.n_slots.
void cluster2_gen::layout_one_lane()
{
    // One-lane pair kernel: the bookkeeping block of a system (16 doubles parked between the tails of two steps) sits at the
    // end of its slab instead of in an array of its own - its address is the slab pointer + a constant, and the register
    // which held it (spilled: two scratch reloads per step) is gone: +0.7 %, profiles/r05_ab_bookkeeping_in_slab.log (a
    // laundered system index in the retire block, against hoisted address arithmetic, measured nothing).
    bk_in_slab = one_lane && !v5_flag("nobkslab");
    if (one_lane) {
        // 32 systems per CU: the slab only keeps the slots which are read through it (positions, products, glue nodes
        // with readers): 63 instead of 144 for the outer Solar System.
        for (std::size_t g = 0; g < pl.groups.size(); ++g) {
            if (grp_natt[g] > 2u) {
                why_not = "one-lane pair kernel: state-variable chains longer than two";
                return;
            }
        }
        // ---- Wide-read layout (round 5). A wavefront pays ~7 cycles of its own time for every LDS instruction it issues
        // (profiles/README.md, issue-rate table), and a round of the step reads 6 positions + 2 x 5 sum operands with 16
        // ds_read_b64. Slots arranged BY CONSUMER make them 10 reads: the three coordinates of a body are adjacent
        // ([x, y, z, -]: one ds_read_b128 + one ds_read_b64 per body), and the five operands of an acceleration sum are
        // adjacent ([t0 .. t4, -]: two ds_read_b128 + one ds_read_b64 per sum, pairs (t0, t1), (t2, t3) as the pairwise sum
        // takes them). A ds_read_b128 moves its 16 bytes per lane at the same LDS-array rate as two ds_read_b64
        // (MI355X_MICROARCH.md, LDS table). The products / reactions of a pair lane now go to the operand arrays of the
        // sums which read them: slot = array of (coordinate i, body) + operand index, with the arrays laid out
        // [coordinate][body] so that the three stores of a lane differ by a constant (one table register for the three).
        // The unused sixth slot of the arrays of the first two bodies takes the stores of the idle lanes. The order of the
        // distance between the slabs of two systems comes out of a scan with the bank model of the guide (reads in the lane
        // groups of each instruction width).
        wide_rd = !v5_flag("nowide") && pp.rx[0] >= 0 && pl.groups.size() == 1u;
        if (wide_rd) {
            std::map<std::uint32_t, std::pair<std::uint32_t, std::uint32_t>> pos_of; // position variable -> (body, coordinate)
            for (std::uint32_t c = 0; c < nc && wide_rd; ++c) {
                for (std::uint32_t sd = 0; sd < 2u; ++sd) {
                    const auto tr = body_vars(c, sd);
                    auto it = std::find(bodies.begin(), bodies.end(), tr);
                    if (it == bodies.end()) {
                        bodies.push_back(tr);
                        it = bodies.end() - 1;
                    }
                    for (std::uint32_t i = 0; i < 3u; ++i) {
                        const auto key = std::make_pair(static_cast<std::uint32_t>(it - bodies.begin()), i);
                        const auto ins = pos_of.emplace(tr[i], key);
                        wide_rd = wide_rd && ins.first->second == key && tr[i] < n_eq && glue_read[tr[i]] != 0;
                    }
                }
            }
            // The sums: one group, all arguments exported cluster outputs, every output read by exactly one sum.
            const auto &grp = pl.groups[0];
            const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
            n_args = static_cast<std::uint32_t>(n0.args.size());
            wide_rd = wide_rd && n0.kind == func_kind::sum && n_args >= 2u && n_args <= 6u;
            std::map<std::uint32_t, std::uint32_t> out_coord; // cluster output -> coordinate
            std::map<std::uint32_t, std::pair<std::uint32_t, bool>> out_src; // cluster output -> (cluster, is reaction)
            for (std::uint32_t c = 0; c < nc; ++c) {
                for (std::uint32_t i = 0; i < 3u; ++i) {
                    out_coord[pl.clusters[c][pp.pr[i]]] = i;
                    out_src[pl.clusters[c][pp.pr[i]]] = {c, false};
                    out_coord[pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])]] = i;
                    out_src[pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])]] = {c, true};
                }
            }
            std::map<std::uint32_t, std::uint32_t> n_readers;
            node_coord.assign(grp.nodes.size(), 0);
            node_rank.assign(grp.nodes.size(), 0);
            // (Signature of a sum: its operands as (cluster, kind) in argument order - the sums of the three coordinates of a
            // body have the same one.)
            std::vector<std::vector<std::pair<std::uint32_t, bool>>> sig(grp.nodes.size());
            for (std::size_t j = 0; j < grp.nodes.size() && wide_rd; ++j) {
                const auto &nd = p.nodes[grp.nodes[j] - n_eq];
                wide_rd = wide_rd && nd.args.size() == n_args;
                for (std::uint32_t a = 0; a < nd.args.size() && wide_rd; ++a) {
                    const auto &o = nd.args[a];
                    wide_rd = wide_rd && is_var(o) && out_coord.count(o.idx) != 0u;
                    if (!wide_rd) {
                        break;
                    }
                    if (a == 0u) {
                        node_coord[j] = out_coord[o.idx];
                    }
                    wide_rd = wide_rd && out_coord[o.idx] == node_coord[j];
                    ++n_readers[o.idx];
                    sig[j].push_back(out_src[o.idx]);
                }
            }
            for (const auto &[u, cnt] : n_readers) {
                (void)u;
                wide_rd = wide_rd && cnt == 1u;
            }
            // Every output which has a slot must have a reader (the others are not stored).
            for (const auto &[u, src_] : out_src) {
                (void)src_;
                wide_rd = wide_rd && (pl.slot_of[u] < 0 || n_readers.count(u) != 0u);
            }
            std::vector<std::vector<std::pair<std::uint32_t, bool>>> ranks;
            for (std::size_t j = 0; j < grp.nodes.size() && wide_rd; ++j) {
                auto it = std::find(ranks.begin(), ranks.end(), sig[j]);
                if (it == ranks.end()) {
                    ranks.push_back(sig[j]);
                    it = ranks.end() - 1;
                }
                node_rank[j] = static_cast<std::uint32_t>(it - ranks.begin());
            }
            n_rank = static_cast<std::uint32_t>(ranks.size());
            // (Three sums per rank, one per coordinate; at least two ranks for the dummy stores.)
            wide_rd = wide_rd && n_rank >= 2u && grp.nodes.size() == 3u * n_rank;
            for (std::uint32_t r = 0; r < n_rank && wide_rd; ++r) {
                std::uint32_t seen = 0;
                for (std::size_t j = 0; j < grp.nodes.size(); ++j) {
                    if (node_rank[j] == r) {
                        seen |= 1u << node_coord[j];
                    }
                }
                wide_rd = wide_rd && seen == 7u;
            }
        }
        // Velocity exchange (round 5). An LDS store is the most expensive instruction of this kernel: 35-40 cycles of the
        // issuing wavefront's time against 5.6 for an FMA (profiles/r05_sensitivity_marginal_costs.log: the store path of
        // a CU moves one ds_write_b64 of a wavefront per ~6 cycles and all eight wavefronts queue on it), and a round stores
        // 3 products + 3 reactions + 2 velocity coefficients (jets) + 2 position coefficients (slab). The position
        // coefficient is the velocity coefficient times RN(1 / (k + 1)): the pair lanes read the velocity jets of their
        // two bodies instead and form d^[k] = (v_a^[k-1] - v_b^[k-1]) RN(1 / k) themselves (one multiplication per
        // coordinate; the order-0 differences come from the current positions), so that the glue lanes neither compute
        // nor store x^[k+1]: 8 stores per round instead of 10. (Rounded once after the subtraction instead of once per body
        // before it: the same quantity to rounding, more accurate where the velocities are close.) Requires the jet
        // columns of the three coordinates of a body to be adjacent: the rows are laid out [system][column] here.
        if (wide_rd && !m4 && !v5_flag("novx")) {
            // Jet column of a velocity variable = index of its glue node in the group (owner slots are filled in that order).
            const auto &grp = pl.groups[0];
            std::map<std::uint32_t, std::uint32_t> col_of_pos; // position variable -> jet column of its velocity
            for (std::size_t j = 0; j < grp.nodes.size(); ++j) {
                const auto it = att.find(grp.nodes[j]);
                if (it != att.end() && it->second.size() == 2u) {
                    col_of_pos[it->second[1]] = static_cast<std::uint32_t>(j);
                }
            }
            vexch = true;
            std::vector<std::uint32_t> body_col(bodies.size(), 0);
            for (std::size_t b = 0; b < bodies.size() && vexch; ++b) {
                for (std::uint32_t i = 0; i < 3u; ++i) {
                    const auto it = col_of_pos.find(bodies[b][i]);
                    vexch = vexch && it != col_of_pos.end() && (i == 0u || it->second == body_col[b] + i);
                    if (vexch && i == 0u) {
                        body_col[b] = it->second;
                    }
                }
            }
            if (vexch) {
                vx_col.assign(pl.L, {});
                for (std::uint32_t l = 0; l < pl.L; ++l) {
                    const auto c = l < nc ? l : 0u;
                    for (std::uint32_t sd = 0; sd < 2u; ++sd) {
                        const auto tr = body_vars(c, sd);
                        vx_col[l][sd] = body_col[static_cast<std::size_t>(std::find(bodies.begin(), bodies.end(), tr) - bodies.begin())];
                    }
                }
            }
        }
        // (The consumer-arranged slots exclude the fused reactions - a product then has two readers -; the analysis above still
        // serves the velocity exchange.)
        const bool wide_an = wide_rd;
        wide_rd = wide_rd && !frx;
        vexch = vexch && wide_an;
        if (lane_sum && !vexch) {
            // (The lane-reduced sums address the jets by column, [system][column]: the layout of the velocity exchange.
            // Without it: the rounds, and the slots numbered after them, as they were.)
            lane_sum = false;
            renumber_sv_slots();
        }
        std::vector<int> remap(pl.n_slots, -1);
        std::uint32_t ns = 0;
        const auto keep = [&](std::uint32_t u) {
            if (pl.slot_of[u] < 0) {
                return false;
            }
            if (pl.cluster_of[u] != -1) {
                // Cluster outputs: the direct products, or - when only the reaction was exported - that one.
                if (fuse_rx && rx_fused[u] != 0) {
                    return pl.slot_of[rx_src[u]] < 0;
                }
                return true;
            }
            // (Velocity exchange: nobody reads a position coefficient through the slab.)
            if (vexch && u < n_eq) {
                return false;
            }
            return glue_read[u] != 0;
        };
        // (The kept slots keep their relative order.)
        std::vector<char> kept(p.n_u, 0);
        std::vector<std::pair<int, std::uint32_t>> order_v;
        for (std::uint32_t u = 0; u < p.n_u; ++u) {
            kept[u] = keep(u) ? 1 : 0;
            if (kept[u] != 0) {
                order_v.emplace_back(pl.slot_of[u], u);
            }
        }
        std::sort(order_v.begin(), order_v.end());
        for (std::uint32_t u = 0; u < p.n_u; ++u) {
            if (kept[u] == 0) {
                pl.slot_of[u] = -1;
            }
        }
        for (const auto &[old_slot, u] : order_v) {
            (void)old_slot;
            if (pl.cluster_of[u] == -1) {
                pl.slot_of[u] = static_cast<int>(ns++);
            }
        }
        // Cluster outputs: every lane (the idle ones too) owns 3 + 3 slots, read or not: lane l keeps its products in the
        // slots out_base + 3 * lane_pr[l] + i and its reactions in rx_base + 3 * lane_rx[l] + i, where lane_pr / lane_rx are
        // permutations of the lanes. The kernel is within 25 % of the LDS throughput, so the permutations and the
        // distance between the slabs of two systems are chosen to minimise the bank conflicts of the exchange (a small
        // deterministic local search over the access patterns of a step; the model is the one of the microarchitecture
        // guide: a ds_read_b64 services the lanes 0-31 / 32-63 together, bank pair = double index mod 32, every further
        // distinct address on a bank pair costs a cycle; a ds_write_b64 services 16 consecutive lanes, double index mod 16).
        const auto out_base = ns;
        const auto rx_base = out_base + 3u * pl.L;
        lane_pr.resize(pl.L);
        lane_rx.resize(pl.L);
        for (std::uint32_t l = 0; l < pl.L; ++l) {
            lane_pr[l] = lane_rx[l] = l;
        }
        // (Fused reactions: the sums read the products; no second region.)
        const bool rx_region = pp.rx[0] >= 0 && !fuse_rx;
        ns = out_base + 3u * pl.L * (rx_region ? 2u : 1u);
        const auto assign = [&]() {
            for (std::uint32_t c = 0; c < nc; ++c) {
                for (std::uint32_t i = 0; i < 3u; ++i) {
                    pl.slot_of[pl.clusters[c][pp.pr[i]]] = static_cast<int>(out_base + 3u * lane_pr[c] + i);
                    if (rx_region) {
                        pl.slot_of[pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])]] = static_cast<int>(rx_base + 3u * lane_rx[c] + i);
                    }
                }
            }
        };
        // Read patterns of a step: per LDS read instruction, the u variable every lane of a group reads.
        std::vector<std::vector<std::uint32_t>> rd_pat;
        for (std::uint32_t i = 0; i < 3u; ++i) {
            for (std::uint32_t sd = 0; sd < 2u; ++sd) {
                std::vector<std::uint32_t> v(pl.L);
                for (std::uint32_t l = 0; l < pl.L; ++l) {
                    v[l] = pl.ext_u[l < nc ? l : 0u][pp.de[i][sd]];
                }
                rd_pat.push_back(std::move(v));
            }
        }
        for (const auto &grp : pl.groups) {
            const auto g = static_cast<std::size_t>(&grp - pl.groups.data());
            const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
            // (A lane-reduced round reads nothing.)
            for (std::uint32_t r = 0; r < (lane_sum && g == 0u ? 1u : n_rounds_of(g)); ++r) {
                for (std::size_t a = 0; a < n0.args.size(); ++a) {
                    if (!is_var(n0.args[a])) {
                        continue;
                    }
                    std::vector<std::uint32_t> v(pl.L);
                    for (std::uint32_t l = 0; l < pl.L; ++l) {
                        v[l] = p.nodes[grp.nodes[round_node(g, r, l).first] - n_eq].args[a].idx;
                        if (fuse_rx && rx_fused[v[l]] != 0) {
                            v[l] = rx_src[v[l]];
                        }
                    }
                    rd_pat.push_back(std::move(v));
                }
            }
        }
        const auto cost = [&](std::uint32_t stride) {
            std::uint64_t tot = 0;
            const auto spw_ = 64u / pl.L;
            // Reads: two groups of 32 lanes.
            for (const auto &v : rd_pat) {
                for (std::uint32_t g = 0; g < 2u; ++g) {
                    std::map<std::uint32_t, std::set<std::uint32_t>> banks;
                    for (std::uint32_t lane = 32u * g; lane < 32u * g + 32u; ++lane) {
                        const auto q = (lane / pl.L) % spw_, l = lane % pl.L;
                        const auto a = q * stride + static_cast<std::uint32_t>(std::max(0, pl.slot_of[v[l]]));
                        banks[a % 32u].insert(a);
                    }
                    std::size_t mx = 1;
                    for (const auto &[b, st_] : banks) {
                        mx = std::max(mx, st_.size());
                    }
                    tot += mx - 1u;
                }
            }
            // Writes of the outputs: four groups of 16 lanes, three coordinates, two kinds.
            for (std::uint32_t kind = 0; kind < (rx_region ? 2u : 1u); ++kind) {
                for (std::uint32_t g = 0; g < 4u; ++g) {
                    std::map<std::uint32_t, std::set<std::uint32_t>> banks;
                    for (std::uint32_t lane = 16u * g; lane < 16u * g + 16u; ++lane) {
                        const auto q = (lane / pl.L) % spw_, l = lane % pl.L;
                        const auto a = q * stride + (kind == 0u ? out_base + 3u * lane_pr[l] : rx_base + 3u * lane_rx[l]);
                        banks[a % 16u].insert(a);
                    }
                    std::size_t mx = 1;
                    for (const auto &[b, st_] : banks) {
                        mx = std::max(mx, st_.size());
                    }
                    tot += 3u * 2u * (mx - 1u); // (a conflicting store costs two LDS cycles more, three coordinates)
                }
            }
            return tot;
        };
        // Total slots incl. the dummy area (as computed below) and the 16 bookkeeping doubles of the system, which sit at the
        // end of its slab (one address register for both: see bk_in_slab).
        const auto n_tot_est = ns + std::max<std::uint32_t>(static_cast<std::uint32_t>(pl.out_pos.size()), 6u) + (bk_in_slab ? 16u : 0u);
        assign();
        slab_stride_opt = n_tot_est;
        auto best = cost(slab_stride_opt);
        for (std::uint32_t st_ = n_tot_est; st_ < n_tot_est + 32u; ++st_) {
            if (const auto c = cost(st_); c < best) {
                best = c;
                slab_stride_opt = st_;
            }
        }
        {
            std::uint64_t rng = 0x9E3779B97F4A7C15ull;
            const auto next = [&]() {
                rng ^= rng << 13;
                rng ^= rng >> 7;
                rng ^= rng << 17;
                return rng;
            };
            for (int it = 0; it < 4000 && best != 0u; ++it) {
                auto &perm = (rx_region && (next() & 1u) != 0u) ? lane_rx : lane_pr;
                const auto i1 = static_cast<std::uint32_t>(next() % pl.L), i2 = static_cast<std::uint32_t>(next() % pl.L);
                if (i1 == i2) {
                    continue;
                }
                std::swap(perm[i1], perm[i2]);
                assign();
                auto c = cost(slab_stride_opt);
                auto cs = slab_stride_opt;
                if (it % 16 == 0) {
                    for (std::uint32_t st_ = n_tot_est; st_ < n_tot_est + 32u; ++st_) {
                        if (const auto c2 = cost(st_); c2 < c) {
                            c = c2;
                            cs = st_;
                        }
                    }
                }
                if (c <= best) {
                    best = c;
                    slab_stride_opt = cs;
                } else {
                    std::swap(perm[i1], perm[i2]);
                }
            }
            assign();
        }
        bank_cost = best;
        pl.n_slots = ns;
        if (wide_rd) {
            place_wide_read_slots();
        }
    }
}

// Stages 2 / 3 up to the glue rounds. Reads pl.n_slots, the slots and the layout decisions; leaves dummy_base, n_slots_tot,
// buf_stride, slab_stride, frx_regs, the division modes of the emitter and the lane tables of the variant: pt (lane pairs),
// st1 (one lane per pair), or ext_tbl / out_tbl / cst_tbl / lane_par_tbls with the operand names they give (pipelined).
void cluster2_gen::lds_layout_and_lane_tables()
{
    // ---- 2. LDS layout: every slot double-buffered by order parity. ----
    const std::uint32_t max_round_outputs = wide_rd ? 2u : std::max<std::uint32_t>(n_out, one_lane ? 6u : 4u);
    dummy_base = pl.n_slots;
    n_slots_tot = pl.n_slots + max_round_outputs;
    // One-lane pair kernel: ONE buffer. A system never spans wavefronts and the LDS instructions of a wavefront complete
    // in order, so a round may overwrite what it has read as long as its reads come first in the instruction stream -
    // which is how the merged schedule is emitted: reads of x^[k] and of the products of order k-1, then the stores of
    // the products of order k and of x^[k+1] (the stores may alias the loads as far as the compiler knows: it keeps
    // their order).
    buf_stride = one_lane ? 0u : n_slots_tot; // doubles between the two parity buffers
    // (One buffer; the stride comes out of the bank-conflict search above.)
    slab_stride = one_lane ? std::max(slab_stride_opt, n_slots_tot + (bk_in_slab ? 16u : 0u))
                                      : ((2u * n_slots_tot) | 1u); // doubles per system
    // (One-lane pair kernel, fused reactions: the coefficients of the sums are loaded once per step - registers through the
    // orders, free again in the tail of the step; "frxlds" among HEYOKA_AMD_V5_OPTS reads them from LDS at every use.)
    frx_regs = frx && !v5_flag("frxlds");
    // Lane-pair kernel: x^[k+1] = f^[k] * RN(1 / (k + 1)) - one multiplication, within 1 ulp of the quotient - instead of
    // the exact 3-operation sequence (60 VALU instructions per step, +2.1 % system-steps/s; the strict-contraction parity
    // test passes its 1e4 / 1e5 eps bounds with it). kw::exact_division restores the correctly-rounded quotient.
    e.recip_div = pairk && !opts.exact_division;
    e.enable_pow_rcp(!opts.exact_division);
    if (pair_split) {
        const auto slot_or = [&](std::uint32_t u, std::uint32_t dflt) {
            return pl.slot_of[u] >= 0 ? static_cast<std::uint32_t>(pl.slot_of[u]) : dflt;
        };
        std::vector<std::uint32_t> s0(L), s1(L), p0(L), p1(L), os_(L), op(L), rs(L), rp(L);
        std::vector<double> csc(L, 1.), crs(L, 0.), crp(L, 0.);
        for (std::uint32_t l = 0; l < L; ++l) {
            const bool valid = l / 2u < nc;
            const auto c = valid ? l / 2u : 0u;
            const bool rb = (l & 1u) != 0u;
            const auto ds = rb ? 2u : 0u;
            const auto &cl = pl.clusters[c];
            const auto ext = [&](std::uint32_t dc, std::uint32_t a) {
                return static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[c][pp.de[dc][a]]]);
            };
            s0[l] = ext(ds, 0);
            s1[l] = ext(ds, 1);
            p0[l] = rb ? s0[l] : ext(1, 0);
            p1[l] = rb ? s0[l] : ext(1, 1);
            if (fuse_rx) {
                os_[l] = valid ? pr_slot(cl[pp.pr[ds]], cl[static_cast<std::uint32_t>(pp.rx[ds])], dummy_base) : dummy_base;
                op[l] = (valid && !rb) ? pr_slot(cl[pp.pr[1]], cl[static_cast<std::uint32_t>(pp.rx[1])], dummy_base + 1u)
                                       : dummy_base + 1u;
            } else {
                os_[l] = valid ? slot_or(cl[pp.pr[ds]], dummy_base) : dummy_base;
                op[l] = (valid && !rb) ? slot_or(cl[pp.pr[1]], dummy_base + 1u) : dummy_base + 1u;
            }
            if (pp.rx[0] >= 0 && !fuse_rx) {
                rs[l] = valid ? slot_or(cl[static_cast<std::uint32_t>(pp.rx[ds])], dummy_base + 2u) : dummy_base + 2u;
                rp[l] = (valid && !rb) ? slot_or(cl[static_cast<std::uint32_t>(pp.rx[1])], dummy_base + 3u) : dummy_base + 3u;
                crs[l] = p.nodes[cl[static_cast<std::uint32_t>(pp.rx[ds])] - n_eq].args[0].value;
                crp[l] = rb ? 0. : p.nodes[cl[static_cast<std::uint32_t>(pp.rx[1])] - n_eq].args[0].value;
            }
            if (pp.sc >= 0) {
                csc[l] = p.nodes[cl[static_cast<std::uint32_t>(pp.sc)] - n_eq].args[0].value;
            }
        }
        pt.s0 = add_utbl(std::move(s0));
        pt.s1 = add_utbl(std::move(s1));
        pt.p0 = add_utbl(std::move(p0));
        pt.p1 = add_utbl(std::move(p1));
        pt.os = add_utbl(std::move(os_));
        pt.op = add_utbl(std::move(op));
        if (pp.rx[0] >= 0 && !fuse_rx) {
            pt.rs = add_utbl(std::move(rs));
            pt.rp = add_utbl(std::move(rp));
            pt.crs = add_dtbl(std::move(crs));
            pt.crp = add_dtbl(std::move(crp));
        }
        if (pp.sc >= 0) {
            pt.csc = add_dtbl(std::move(csc));
        }
    }
    if (one_lane) {
        std::vector<double> csc(L, 1.), crs(L, 0.);
        for (std::uint32_t i = 0; i < 3u; ++i) {
            std::vector<std::uint32_t> s0(L), s1(L), o(L), r(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                const bool valid = l < nc;
                const auto c = valid ? l : 0u;
                const auto &cl = pl.clusters[c];
                if (vexch) {
                    // (Velocity exchange: the jet columns of the two bodies instead of slab slots.)
                    s0[l] = vx_col[l][0] + i;
                    s1[l] = vx_col[l][1] + i;
                } else {
                    s0[l] = static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[c][pp.de[i][0]]]);
                    s1[l] = static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[c][pp.de[i][1]]]);
                }
                // (Every lane owns its output slots, the idle ones too: slot = first slot of pair 0 + 3 * lane + i.)
                o[l] = wide_rd ? wide_pr[l][i]
                               : static_cast<std::uint32_t>(pl.slot_of[pl.clusters[0][pp.pr[i]]]) - 3u * lane_pr[0] + 3u * lane_pr[l];
                if (pp.rx[0] >= 0 && !fuse_rx) {
                    const auto ru = cl[static_cast<std::uint32_t>(pp.rx[i])];
                    r[l] = wide_rd ? wide_rx[l][i]
                                   : static_cast<std::uint32_t>(pl.slot_of[pl.clusters[0][static_cast<std::uint32_t>(pp.rx[i])]])
                                         - 3u * lane_rx[0] + 3u * lane_rx[l];
                    const auto cv = p.nodes[ru - n_eq].args[0].value;
                    if (i > 0u && cv != crs[l]) {
                        why_not = "one-lane pair kernel: the reaction coefficients of a pair differ between the coordinates";
                        return;
                    }
                    crs[l] = cv;
                }
                if (pp.sc >= 0) {
                    csc[l] = p.nodes[cl[static_cast<std::uint32_t>(pp.sc)] - n_eq].args[0].value;
                }
            }
            st1.s[i][0] = add_utbl(std::move(s0));
            st1.s[i][1] = add_utbl(std::move(s1));
            st1.o[i] = add_utbl(std::move(o));
            if (pp.rx[0] >= 0 && !fuse_rx) {
                st1.r[i] = add_utbl(std::move(r));
            }
        }
        if (pp.sc >= 0) {
            st1.csc = add_dtbl(std::move(csc));
        }
        if (pp.rx[0] >= 0 && !fuse_rx) {
            st1.crs = add_dtbl(std::move(crs));
        }
    }
    ext_tbl.assign(n_ext, 0), out_tbl.assign(n_out, 0), cst_tbl.assign(n_cst, 0);
    for (std::uint32_t x = 0; !pairk && x < n_ext; ++x) {
        std::vector<std::uint32_t> v(L);
        for (std::uint32_t l = 0; l < L; ++l) {
            v[l] = static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[l < nc ? l : 0u][x]]);
        }
        ext_tbl[x] = add_utbl(std::move(v));
    }
    for (std::uint32_t x = 0; !pairk && x < n_out; ++x) {
        std::vector<std::uint32_t> v(L);
        for (std::uint32_t l = 0; l < L; ++l) {
            v[l] = l < nc ? static_cast<std::uint32_t>(pl.slot_of[pl.clusters[l][pl.out_pos[x]]]) : dummy_base + x;
        }
        out_tbl[x] = add_utbl(std::move(v));
    }
    for (std::uint32_t x = 0; !pairk && x < n_cst; ++x) {
        std::vector<double> v(L);
        for (std::uint32_t l = 0; l < L; ++l) {
            v[l] = pl.cst_val[l < nc ? l : 0u][x];
        }
        cst_tbl[x] = add_dtbl(std::move(v));
        const auto [q, a] = pl.cst_pos[x];
        e.numpar_override[&p.nodes[t0()[q] - n_eq].args[a]] = "ccst" + std::to_string(x);
    }
    for (std::size_t x = 0; !pairk && x < pl.par_pos.size(); ++x) {
        std::vector<std::uint32_t> v(L);
        for (std::uint32_t l = 0; l < L; ++l) {
            v[l] = pl.par_idx[l < nc ? l : 0u][x];
        }
        const auto [q, a] = pl.par_pos[x];
        e.numpar_override[&p.nodes[t0()[q] - n_eq].args[a]] = lane_par(std::move(v));
    }
}

// Reads the plan, att, the slots and the fusion flags; leaves rounds (with their tables and owner slots), n_own and the
// numbers of jet columns n_col / n_dcol.
void cluster2_gen::build_glue_rounds()
{
    rounds.assign(pl.groups.size(), {});
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &grp = pl.groups[g];
        const auto n_rounds = n_rounds_of(g);
        const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
        for (std::uint32_t r = 0; r < n_rounds; ++r) {
            glue_round gr;
            const bool mapped = lane_sum && g == 0u;
            // (Which lanes own a node of the round.)
            std::uint32_t valid_mask = 0;
            for (std::uint32_t l = 0; l < L; ++l) {
                valid_mask |= round_node(g, r, l).second ? (1u << l) : 0u;
            }
            const auto is_valid = [&](std::uint32_t l) { return (valid_mask >> l & 1u) != 0u; };
            gr.n_valid = static_cast<std::uint32_t>(__builtin_popcount(valid_mask));
            // (Lane-reduced round: the sums come out of the registers of the first round, see emit_glue_compute().)
            gr.reduced = mapped && r == 1u;
            const auto node_of = [&](std::uint32_t l) { return grp.nodes[round_node(g, r, l).first]; };
            bool round_fused = false;
            for (std::uint32_t l = 0; fuse_rx && l < L; ++l) {
                for (const auto &o : p.nodes[node_of(l) - n_eq].args) {
                    round_fused = round_fused || (is_var(o) && rx_fused[o.idx] != 0);
                }
            }
            for (std::size_t a = 0; a < n0.args.size() && !gr.reduced; ++a) {
                if (is_var(n0.args[a]) && round_fused) {
                    std::vector<std::uint32_t> v(L);
                    std::vector<double> cf(L, 1.);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        const auto ua = p.nodes[node_of(l) - n_eq].args[a].idx;
                        if (rx_fused[ua] != 0) {
                            v[l] = pr_slot(rx_src[ua], ua, 0);
                            cf[l] = p.nodes[ua - n_eq].args[0].value;
                        } else {
                            v[l] = static_cast<std::uint32_t>(pl.slot_of[ua]);
                        }
                    }
                    gr.arg_tbl.push_back(add_utbl(std::move(v)));
                    gr.coef_tbl.push_back(add_dtbl(std::move(cf)));
                } else if (is_var(n0.args[a])) {
                    std::vector<std::uint32_t> v(L);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        v[l] = static_cast<std::uint32_t>(pl.slot_of[p.nodes[node_of(l) - n_eq].args[a].idx]);
                    }
                    gr.arg_tbl.push_back(add_utbl(std::move(v)));
                } else if (n0.args[a].type == operand::kind::num) {
                    std::vector<double> v(L);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        v[l] = p.nodes[node_of(l) - n_eq].args[a].value;
                    }
                    gr.arg_tbl.push_back(add_dtbl(std::move(v)));
                } else {
                    // Parameter: per-lane index (the nodes of a group may read different parameters).
                    std::vector<std::uint32_t> v(L);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        v[l] = p.nodes[node_of(l) - n_eq].args[a].idx;
                    }
                    gr.par_name.resize(n0.args.size());
                    gr.par_name[a] = lane_par(std::move(v));
                    gr.arg_tbl.push_back(0);
                }
            }
            bool any_read = false;
            std::vector<std::uint32_t> v(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                const auto u = node_of(l);
                v[l] = (is_valid(l) && pl.slot_of[u] >= 0) ? static_cast<std::uint32_t>(pl.slot_of[u]) : dummy_base;
                any_read = any_read || (is_valid(l) && glue_read[u] != 0);
            }
            gr.exported = any_read;
            gr.out_tbl = add_utbl(std::move(v));
            for (std::uint32_t a = 0; a < grp_natt[g]; ++a) {
                owner_slot ow;
                std::vector<std::uint32_t> vs(L), vv(L);
                for (std::uint32_t l = 0; l < L; ++l) {
                    const auto var = att.at(node_of(l))[a];
                    vs[l] = (is_valid(l) && pl.slot_of[var] >= 0) ? static_cast<std::uint32_t>(pl.slot_of[var]) : dummy_base;
                    vv[l] = var;
                }
                if (mapped) {
                    // (Jet column of a node = its index in the group: the columns stay in the order of the nodes, whichever
                    // lane computes them.)
                    std::vector<std::uint32_t> vc(L);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        vc[l] = round_node(g, r, l).first;
                    }
                    ow.mapped = true;
                    ow.reduced = gr.reduced;
                    ow.col_tbl = add_utbl(std::move(vc), false);
                    ow.valid_mask = valid_mask;
                }
                ow.out_tbl = add_utbl(std::move(vs));
                ow.var_tbl = add_utbl(std::move(vv), false);
                ow.col = n_own++;
                ow.n_valid = gr.n_valid;
                if (one_lane && a >= 1u) {
                    ow.derived = true;
                    ow.parent = gr.owners[a - 1u].col;
                    ow.cbase = n_dcol;
                    n_dcol += gr.n_valid;
                } else {
                    ow.cbase = n_col;
                    n_col += gr.n_valid;
                }
                ow.xname.resize(order + 1u);
                ow.slab_needed = false;
                for (std::uint32_t l = 0; l < L; ++l) {
                    ow.slab_needed = ow.slab_needed || (is_valid(l) && glue_read[att.at(node_of(l))[a]] != 0);
                }
                // (Velocity exchange: nobody reads a position coefficient - the compiler drops the unused ones.)
                ow.slab_needed = ow.slab_needed && !vexch;
                gr.owners.push_back(std::move(ow));
            }
            rounds[g].push_back(std::move(gr));
        }
    }
    if (n_own == 0u) {
        why_not = "no state variable could be attached to a glue round";
        return;
    }
}

// Reads rounds, the columns, the geometry and slab_stride; leaves the layout of the jets (n_colp, n_dcolp, n_hslots,
// jet_rows_doubles, jet_doubles_per_wave), jet_lds and what follows from it (tables_of_the_jet_placement()), merged.
void cluster2_gen::layout_jets_and_schedule()
{
    n_colp = one_lane ? n_col : n_col + 1u;
    n_dcolp = one_lane ? n_dcol : n_dcol + 1u;
    n_hslots = (n_col + L - 1u) / L; // lane slots of the final Horner / compensated evaluation
    // Jets of the state variables: [order][system of the wave][column], per wave. Kept in LDS when the
    // block's slab + jets fit in the 160 KB of a CU (the kernel occupies a whole CU anyway: 512 registers
    // per lane), otherwise in a per-wave global scratch.
    jet_rows_doubles = static_cast<std::uint64_t>(order + 1u) * spw * n_colp;
    jet_doubles_per_wave = jet_rows_doubles + (one_lane ? static_cast<std::uint64_t>(spw) * n_dcolp : 0u);
    // The LDS budget rule: the layout with the jets in LDS is built first - everything hy_taylor declares in LDS
    // follows from it: the tables of the packed final evaluation, the rows of the mode-4 store - and kept when the
    // footprint of ALL those arrays (lds_arrays(), which text_kernel_prologue() declares them from) fits in the LDS of a
    // CU; otherwise it is taken back and the layout with the jets in global scratch is held to the same limit.
    const auto n_ut_before = utbl.size();
    jet_lds = true;
    tables_of_the_jet_placement();
    if (lds_footprint() > lds_limit_bytes) {
        const auto with_jets = lds_footprint();
        utbl.resize(n_ut_before), utexpr.resize(n_ut_before), utbl_is_slot.resize(n_ut_before);
        pk_tbl.clear();
        jet_lds = false;
        tables_of_the_jet_placement();
        detail::log_message(log_level::debug, "cluster kernel, " + std::to_string(L) + " lanes per system, order " + std::to_string(order)
                                                  + ": with the jets in LDS the kernel would declare " + std::to_string(with_jets)
                                                  + " bytes of LDS (limit " + std::to_string(lds_limit_bytes) + "): jets in global scratch, "
                                                  + std::to_string(lds_footprint()) + " bytes");
    }
    if (lds_footprint() > lds_limit_bytes) {
        why_not = "the slab and the lane tables of the systems of a CU (" + std::to_string(lds_footprint()) + " bytes) do not fit in its LDS ("
                  + std::to_string(lds_limit_bytes) + " bytes)";
        res.more_lanes_cure = one_lane;
        return;
    }
    if (vexch && (!jet_lds || n_dcol != n_col)) {
        why_not = "one-lane pair kernel: the velocity exchange needs the jets in LDS and one position per velocity";
        res.more_lanes_cure = true;
        return;
    }

    // Merged schedule (lane-pair variant, one glue level after the clusters): round k = cluster(k) + glue(k-1),
    // one LDS synchronisation per order instead of two.
    merged = pairk && pl.cluster_level == 1u && pl.max_level == 2u
             && std::all_of(pl.groups.begin(), pl.groups.end(), [](const auto &g) { return g.level == 2u; });
    if (one_lane && !merged) {
        why_not = "one-lane pair kernel: the merged schedule does not apply";
        return;
    }
}

// What follows from where the jets live (jet_lds): compact_tc, pk_tbl (three more tables per packed owner slot) and
// n_tc_rows - after it the tables are complete, and with them the LDS arrays of the kernel.
void cluster2_gen::tables_of_the_jet_placement()
{
    // Stepper with events: compact set of Taylor coefficients (see emitted_module::compact_tc) through the cooperative
    // store of the LDS-resident jets. HEYOKA_AMD_COMPACT_TC=0 switches it off (A/B measurements).
    compact_tc = [&]() {
        if (!m4 || !jet_lds) {
            return false;
        }
        if (one_lane) {
            return true;
        }
        if (!opts.dev.compact_tc) {
            return false;
        }
        // (Chains x' = v, v' = a only: the parent of a derived variable is not derived itself.)
        const auto derived = [&](std::uint32_t var) { return emit_detail::defined_by_state_variable(p, var); };
        bool any = false;
        for (std::uint32_t var = 0; var < n_eq; ++var) {
            if (derived(var)) {
                if (derived(p.sv_defs[var].idx)) {
                    return false;
                }
                any = true;
            }
        }
        return any;
    }();
    for_each_owner([&](auto &gr, auto &ow) {
        for (const auto &o2 : gr.owners) {
            if (!(o2.derived && o2.parent == ow.col && pack_tail_slot(ow, &o2))) {
                continue;
            }
            const auto nv = ow.n_valid;
            const auto kst = static_cast<std::uint64_t>(spw) * n_colp;
            std::vector<std::uint32_t> tv(L), tj(L), tf(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                const bool isx = l >= nv && l < 2u * nv;
                const auto c = isx ? l - nv : (l < nv ? l : 0u);
                tv[l] = static_cast<std::uint32_t>((isx ? jet_rows_doubles + jet_off(o2) : jet_off(ow)) + c);
                tj[l] = static_cast<std::uint32_t>(jet_off(ow) + c + (isx ? 0u : kst));
                tf[l] = isx ? order + 1u : 0u;
            }
            pk_tbl[ow.col] = {add_utbl(std::move(tv), false), add_utbl(std::move(tj), false), add_utbl(std::move(tf), false)};
        }
    });
    // Rows of the cooperative store of the Taylor coefficients (mode 4; the table itself: text_helpers_and_constant_tables()):
    // order + 1 per state variable, one for a variable which leaves with its order-0 row only.
    n_tc_rows = 0;
    if (m4 && one_lane) {
        for_each_owner([&](auto &, auto &ow) { n_tc_rows += static_cast<std::size_t>(ow.n_valid) * (ow.derived ? 1u : order + 1u); });
    } else if (m4) {
        for (std::uint32_t var = 0; var < n_eq; ++var) {
            n_tc_rows += (compact_tc && emit_detail::defined_by_state_variable(p, var)) ? 1u : order + 1u;
        }
    }
}

// Every array which hy_taylor declares in LDS, in the order of the declarations: text_kernel_prologue() takes the sizes from
// here, layout_jets_and_schedule() the decision where the jets live. Reads the geometry, the layout and the tables.
std::vector<cluster2_gen::lds_array> cluster2_gen::lds_arrays() const
{
    std::vector<lds_array> out;
    out.push_back({"lds_slab", 8u, static_cast<std::uint64_t>(wpb) * spw * slab_stride});
    if (one_lane && !bk_in_slab) {
        out.push_back({"lds_bk", 8u, static_cast<std::uint64_t>(wpb) * spw * 16u});
    }
    if (jet_lds) {
        out.push_back({"lds_jet", 8u, wpb * jet_doubles_per_wave});
        if (m4) {
            out.push_back({"lds_tcsrc", 8u, std::max<std::uint64_t>(n_tc_rows, 1u)});
        }
    }
    out.push_back({"lds_utbl", 2u, std::max<std::uint64_t>(utbl.size(), 1u) * L});
    if (one_lane) {
        out.push_back({"lds_dt", 8u, std::max<std::uint64_t>(dtbl.size(), 1u) * L});
    }
    if (!pk_tbl.empty()) {
        out.push_back({"lds_fac", 8u, 2u * (order + 1u)});
    }
    return out;
}

// Bytes of LDS of a workgroup of hy_taylor: the arrays, each rounded up to the strictest alignment any of them asks for (16
// bytes, the slab of the wide-read layout) - the compiler is free in how it orders them.
std::uint64_t cluster2_gen::lds_footprint() const
{
    std::uint64_t n = 0;
    for (const auto &a : lds_arrays()) {
        n += (a.count * a.elem_bytes + 15u) / 16u * 16u;
    }
    return n;
}

std::uint64_t cluster2_gen::lds_count(const char *name) const
{
    for (const auto &a : lds_arrays()) {
        if (std::string(a.name) == name) {
            return a.count;
        }
    }
    throw std::logic_error(std::string("no LDS array ") + name);
}

// The state of the order programs. Reads the variant, opts and the plan; leaves t0_ids, the (empty) coefficient histories
// of the pair programs, the padding counts and switches of the one-lane program, and ext_const.
void cluster2_gen::init_order_programs()
{
    for (const auto u : t0()) {
        t0_ids.push_back(u - n_eq);
    }
    aP.assign(order + 1u, {}), aR.assign(order + 1u, {}), aRp.assign(order + 1u, {}), aS.assign(order + 1u, {});
    has_rx = pp.rx[0] >= 0;
    // Normalised pow recurrence (default): lane B keeps b_k / b_0 (k >= 1) instead of b_k, one multiplication by
    // RN(1 / b_0) folded into the FMA which forms the lane's aP[k]; the recurrence k b_0 a_k = sum(...) then needs no
    // division: a_k = alpha S1 - (alpha + 1) S2 / k on the normalised sums. The new coefficient goes to both lanes of
    // the pair with one DPP broadcast from the odd lane. kw::exact_division: the quotient by b_0 with a Markstein
    // correction, within 1.5 ulp of the reference's single division.
    pow_norm = !opts.exact_division;
    sB.assign(order + 1u, {}), sA.assign(order + 1u, {});
    for (auto &v : sD) {
        v.resize(order + 1u);
    }
    // Sensitivity experiment (profiles/experiments/sensitivity.py): HEYOKA_AMD_V5_PAD = "chain:dep:st:ld:salu" adds that many
    // dummy instructions of each kind to every order - independent FMAs in the chain section, dependent FMAs, LDS stores
    // and LDS reads in the dependent section, scalar no-ops - without touching the results: the slope of the step time
    // against each count says which resource the kernel is bound by.
    // (A sixth field: that many per-lane doubles kept live through the step, each used by one dependent FMA per order - what
    // per-lane coefficients of the acceleration sums would cost in registers; "norx" among HEYOKA_AMD_V5_OPTS drops the
    // reaction products and their stores - WRONG results, timing only: what fusing them into the sums could gain.)
    if (!opts.dev.v5_pad.empty()) {
        std::sscanf(opts.dev.v5_pad.c_str(), "%u:%u:%u:%u:%u:%u", &pad_chain, &pad_dep, &pad_st, &pad_ld, &pad_salu, &pad_regs);
    }
    any_pad = (pad_chain | pad_dep | pad_st | pad_ld | pad_salu | pad_regs) != 0u;
    exp_norx = v5_flag("norx");
    // One accumulator for the half sum of squares bh_k = sum_i (sum_j d_i[k-j] d_i[j] + 1/2 d_i[k/2]^2): the three chains
    // of the coordinates run into each other - two additions per order and two multiply-adds per even order less, two
    // accumulators less. (The reference adds the three squares pairwise, src/detail/sum_sq.cpp:120-245: same terms, other
    // rounding order - inside the stated tolerances like the suffix sums of the pow recurrence.)
    merged_sq = !v5_flag("nomsq");
    sel_scalar = one_lane && !v5_flag("nosc");
    // Issue priority (s_setprio): raised between the LDS exchange and the end of the finishing operations of a round - the
    // dependent chain which decides how soon the next exchange can start - and lowered for the convolution chains, so
    // that the wavefront which is in its critical section wins the VALU over the one streaming FMAs.
    // Measured (outer Solar System, 1 048 576 systems, A/B harness): 7.02e8 -> 7.15e8 system-steps/s; on by default,
    // HEYOKA_AMD_V5_PRIO=0 switches it off, =2 also keeps the serial tail of the step at the high priority.
    prio_mode = opts.dev.v5_prio;
    prio_switch = prio_mode != 0;
    // External inputs which are constant u variables in EVERY cluster (isomorphic clusters may pair a constant with a
    // variable: the heliocentric alias x_i - 0 and the pair difference x_j - x_i of model::np1body).
    ext_const.assign(n_ext, 1);
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        for (std::size_t c = 0; c < nc; ++c) {
            ext_const[x] = (ext_const[x] != 0 && cu[pl.ext_u[c][x]] != 0) ? 1 : 0;
        }
    }
}

// Reads everything before it; leaves the statements of one step in body (and os empty), the SSA names of the coefficients
// in the owner slots (publish_sv) and in the histories, and e.n_stmt.
void cluster2_gen::emit_step_body()
{
    // ===================== step body =====================
    os << "double m0 = 0.0, mo = 0.0, mom1 = 0.0;\n";
    if (frx_regs) {
        for (const auto &rg : rounds) {
            for (const auto &gr : rg) {
                for (const auto t : gr.coef_tbl) {
                    os << "const double frc" << t << " = " << dtname(t) << ";\n";
                }
            }
        }
    }
    if (one_lane && !opts.dev.v5_pad.empty()) {
        os << "double hy_pad0 = 1.0, hy_pad1 = 1.0, hy_pad2 = 1.0, hy_pad3 = 1.0, hy_pad4 = 1.0;\n";
        unsigned n_rp = 0;
        std::sscanf(opts.dev.v5_pad.c_str(), "%*u:%*u:%*u:%*u:%*u:%u", &n_rp);
        for (unsigned i = 0; i < n_rp; ++i) {
            os << "double hy_rp" << i << " = lds_fac[(threadIdx.x + " << i << "u) % 40u];\n";
        }
    }
    for_each_owner([&](auto &, auto &ow) {
        os << "const double xs" << ow.col << " = " << row0_r(ow) << ";\n";
        publish_sv(ow, 0, "xs" + std::to_string(ow.col));
    });
    // (One-lane pair kernel, single-buffered slab: the order-1 coefficients go to the slab once the order-0 ones have
    // been read, i.e. after the reads of round 0.)
    std::vector<std::tuple<owner_slot *, std::uint32_t, std::string>> deferred_pub;
    if (merged) {
        // Orders 1 .. a of the a-th variable of a chain follow from the state alone.
        for (auto &rg : rounds) {
            for (auto &gr : rg) {
                for (std::size_t a = 1; a < gr.owners.size(); ++a) {
                    for (std::uint32_t j = 1; j <= a && j <= order; ++j) {
                        const auto x = e.div_const(gr.owners[a - 1u].xname[j - 1u], j);
                        if (one_lane) {
                            deferred_pub.emplace_back(&gr.owners[a], j, x);
                        } else {
                            publish_sv(gr.owners[a], j, x);
                        }
                    }
                }
            }
        }
    }
    sync();
    for (std::uint32_t k = 0; merged && k <= order; ++k) {
        std::vector<std::string> prd;
        if (k < order) {
            prd = one_lane ? emit_single_reads(k) : emit_pair_reads(k);
        }
        if (k == 0u) {
            for (auto &[ow, j, x] : deferred_pub) {
                publish_sv(*ow, j, x);
            }
        }
        std::vector<std::tuple<std::size_t, std::uint32_t, std::vector<std::string>>> pend;
        if (k >= 1u) {
            for (std::size_t g = 0; g < pl.groups.size(); ++g) {
                for (std::uint32_t r = 0; r < rounds[g].size(); ++r) {
                    pend.emplace_back(g, r, emit_glue_reads(g, r, k - 1u));
                }
            }
        }
        if (one_lane) {
            // Round k of the one-lane kernel: LDS reads | early chains of order k + 1 (independent of the reads) | glue of
            // order k - 1 (consumes its ten operands right away: 20 registers which would otherwise stay live across
            // the finishing operations of the pairs) | finishing of order k, stores, late chains.
            if (prio_switch) {
                os << "__builtin_amdgcn_s_setprio(3);\n";
            }
            sched_fence();
            if (k < order) {
                sched_fence();
            }
            if (lane_sum && k >= 1u) {
                // The lane-reduced round first: its terms are one operand of the first round, and its lanes without a sum
                // store their partial sums to a jet column of the FIRST round (ls_park), which the store of that round - the
                // next LDS instruction of the wavefront to that address: they complete in order - overwrites with the
                // coefficient. (The jets have no spare column, and a select of the address would cost every order.)
                emit_glue_compute(0, 1, k - 1u, {std::get<2>(pend[0]).at(ls_pos)});
                emit_glue_compute(0, 0, k - 1u, std::get<2>(pend[0]));
            } else {
                for (const auto &[g, r, names] : pend) {
                    emit_glue_compute(g, r, k - 1u, names);
                }
            }
            if (k < order) {
                emit_single_compute(k, prd);
            }
            if (k < order) {
                emit_single_history(k);
            }
            if (prio_switch && k == order && prio_mode != 2) {
                os << "__builtin_amdgcn_s_setprio(0);\n";
            }
            sync();
            continue;
        }
        if (k < order) {
            emit_pair_compute(k, prd);
        }
        for (const auto &[g, r, names] : pend) {
            emit_glue_compute(g, r, k - 1u, names);
        }
        sync();
    }
    for (std::uint32_t k = 0; !merged && k < order; ++k) {
        for (std::uint32_t lev = 1; lev <= pl.max_level; ++lev) {
            if (lev == pl.cluster_level) {
                emit_cluster(k);
            }
            const bool last = (lev == pl.max_level);
            if (overlap && last) {
                // Reads of all the rounds of the level first, then the independent chunk, then the computations.
                std::vector<std::tuple<std::size_t, std::uint32_t, std::vector<std::string>>> pend;
                for (std::size_t g = 0; g < pl.groups.size(); ++g) {
                    if (pl.groups[g].level == lev) {
                        for (std::uint32_t r = 0; r < rounds[g].size(); ++r) {
                            pend.emplace_back(g, r, emit_glue_reads(g, r, k));
                        }
                    }
                }
                if (!pair_split) {
                    sched_fence();
                    e.emit_partials_sel(t0_ids, k + 1u, psel::late);
                    e.emit_partials_sel(t0_ids, k + 2u, psel::early_a);
                    if (fence2) {
                        sched_fence();
                    }
                }
                for (const auto &[g, r, names] : pend) {
                    emit_glue_compute(g, r, k, names);
                }
            } else {
                for (std::size_t g = 0; g < pl.groups.size(); ++g) {
                    if (pl.groups[g].level == lev) {
                        for (std::uint32_t r = 0; r < rounds[g].size(); ++r) {
                            emit_glue_round(g, r, k);
                        }
                    }
                }
                if (!pair_split && !overlap && last && k + 1u < order) {
                    // History part of the next order's convolutions: overlaps the exchange latency.
                    e.emit_partials(t0_ids, k + 1u, 0, n_parts);
                }
            }
            sync();
        }
    }
    if (one_lane && !opts.dev.v5_pad.empty()) {
        os << "asm volatile(\"\" ::\"v\"(hy_pad4));\n";
    }
    body = os.str();
    os.str("");
    os.clear();
}

// Reads the variant, the tables, rounds and the jet layout; leaves the defines, the prelude, the __device__ helpers of the
// variant and the __constant__ tables in src, and n_tc_rows (refusals: overflows of the table entries).
void cluster2_gen::text_helpers_and_constant_tables()
{
    // NOTE: a local search over slot permutations minimising the LDS bank conflicts of the gather-type reads
    // was tried and removed: it lowered SQ_LDS_BANK_CONFLICT by 9 % with no change in kernel time. A
    // microbenchmark on gfx950 shows why: a single wavefront issues one ds_read_b64 per 6.6 clk whatever the
    // pattern (consecutive, 2-way conflicting, strided groups), only a 64-way same-bank pattern is slower
    // (34.6 clk); the cost of the LDS traffic here is the issue slots of its ~620 instructions per step.

    // ===================== module text =====================
    src << "#define SPW " << spw << "u\n#define HY_WPB " << wpb << "u\n";
    src << "#define HY_M4 " << (m4 ? 1 : 0) << "\n";
    // (The stepper with events is a specialisation of its own and always runs in mode 4: a compile-time constant there - the
    // bookkeeping of the propagation mode, ~900 instructions per group of systems around a single step, is not generated.)
    src << "#define HY_MODE " << (m4 ? "4" : "a.mode") << "\n";
    // (Propagation from grid point to grid point: see hy_kargs::tc_thr.)
    src << "#define HY_GRID_STOP " << ((one_lane && jet_lds && !m4) ? "((HY_MODE == 1) & ((a.pad & 4) != 0) & hy_reach)" : "false") << "\n";
    src << "#define HY_GRID_FLAGS " << ((one_lane && jet_lds && !m4) ? "((HY_MODE == 1) & ((a.pad & 4) != 0))" : "false") << "\n";
    // (The stepper with events always uses the static schedule: its cooperative store has workgroup barriers.)
    src << "#define HY_NO_STATIC 0\n";
    src << prelude();
    emit_detail::emit_dout(src, p, opts);
    src << emit_detail::wsync_macro;
    src << R"HIP(
// Maximum of the norm accumulators. They start from 0.0 and (a < b) ? b : a never selects a NaN b: the first operand
// is never a NaN, and for such operands the IEEE maximum (one instruction: it returns the non-NaN operand) is the same
// function as the comparison + select of hy_max(). (Written as the instruction itself: fmax() would first canonicalise
// every operand which comes out of a lane exchange, one more v_max_f64 each.)
__device__ __forceinline__ double hy_nmax(double a, double b)
{
#if defined(HY_NO_NMAX)
    return hy_max(a, b);
#else
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
#endif
}
// A product which is never contracted into an FMA with its consumer (the value must be the ROUNDED product).
__device__ __forceinline__ double hy_mul_nc(double x, double y)
{
    double t = x * y;
    asm("" : "+v"(t));
    return t;
}
template <int CTRL>
__device__ __forceinline__ double hy_dpp(double x)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
)HIP";
    // (hy_sel_log(): the logarithm of the step-size selector, in the common prelude - hip_emit.cpp.)
    if (wide_rd) {
        // (The native vector type: a load of HIP's double2 - a struct - is taken apart into two 8-byte loads by SROA.)
        src << "#if defined(HY_HOST_EMU)\nstruct hy_d2 {\n    double x, y;\n};\n#else\n"
               "typedef double hy_d2 __attribute__((ext_vector_type(2)));\n#endif\n";
    }
    if (one_lane) {
        // The logarithm and the exponential of the selector with their polynomial constants in SCALAR registers. A Horner
        // step p * w + C with a literal C compiles to v_mov_b32 x 2 (the literal into the destination pair) + v_fmac_f64:
        // three VALU instructions where v_fma_f64 with C in an SGPR pair is one - VOP3 takes no 64-bit literal, and the
        // instruction selector prefers the two-address form even when the constant already sits in scalar registers, hence
        // the instruction is written out (hy_fma_sc). The constants are materialised by s_mov_b32 pairs next to their use
        // (MachineLICM is off for this module), which issue on the scalar unit next to the other wavefront's arithmetic: 39 VALU instructions per step less (20 in the logarithm, 19 against the device library's
        // exp(), whose minimax polynomial has the same shape). hy_sel_exp_s(): k = rint(x / ln 2), r = x - k ln 2 in two
        // pieces, Taylor polynomial of degree 13 on |r| <= 0.347 (truncation 4e-18), ldexp; +inf -> +inf, -inf -> 0, nan -> nan.
        src << R"HIP(
#if defined(HY_HOST_EMU)
#define hy_fma_sc(a, b, c) __builtin_fma((a), (b), (c))
#else
// a * b + c with the (uniform) addend c in a scalar register pair: ONE v_fma_f64.
__device__ __forceinline__ double hy_fma_sc(double a, double b, double c)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}
#endif
__device__ __forceinline__ double hy_sel_log_s(double x)
{
    double m = __builtin_amdgcn_frexp_mant(x);
    int e = __builtin_amdgcn_frexp_exp(x);
    const bool lo = m < 0x1.6a09e667f3bcdp-1;
    m = m * (lo ? 2.0 : 1.0);
    e -= lo ? 1 : 0;
    const double num = m - 1.0, den = m + 1.0;
    double r = __builtin_amdgcn_rcp(den);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    double z = num * r;
    z = __builtin_fma(__builtin_fma(-den, z, num), r, z);
    const double w = z * z;
    double p = __builtin_fma(w, 0x1.8618618618618p-4, 0x1.af286bca1af28p-4);
    p = hy_fma_sc(p, w, 0x1.e1e1e1e1e1e1ep-4);
    p = hy_fma_sc(p, w, 0x1.1111111111111p-3);
    p = hy_fma_sc(p, w, 0x1.3b13b13b13b14p-3);
    p = hy_fma_sc(p, w, 0x1.745d1745d1746p-3);
    p = hy_fma_sc(p, w, 0x1.c71c71c71c71cp-3);
    p = hy_fma_sc(p, w, 0x1.2492492492492p-2);
    p = hy_fma_sc(p, w, 0x1.999999999999ap-2);
    p = hy_fma_sc(p, w, 0x1.5555555555555p-1);
    const double ed = (double)e;
    double res = __builtin_fma(ed, 0x1.abc9e3b39803fp-56, (z * w) * p);
    res = __builtin_fma(2.0, z, res);
    res = __builtin_fma(ed, 0x1.62e42fefa39efp-1, res);
    res = (x == 0.0) ? -__builtin_inf() : res;
    res = (x == __builtin_inf()) ? x : res;
    return res;
}
__device__ __forceinline__ double hy_sel_exp_s(double x)
{
    const double kf = __builtin_rint(x * 0x1.71547652b82fep+0);
    double r = __builtin_fma(kf, -0x1.62e42fefa39efp-1, x);
    r = __builtin_fma(kf, -0x1.abc9e3b39803fp-56, r);
    double p = __builtin_fma(r, 0x1.6124613a86d09p-33, 0x1.1eed8eff8d898p-29);
    p = hy_fma_sc(p, r, 0x1.ae64567f544e4p-26);
    p = hy_fma_sc(p, r, 0x1.27e4fb7789f5cp-22);
    p = hy_fma_sc(p, r, 0x1.71de3a556c734p-19);
    p = hy_fma_sc(p, r, 0x1.a01a01a01a01ap-16);
    p = hy_fma_sc(p, r, 0x1.a01a01a01a01ap-13);
    p = hy_fma_sc(p, r, 0x1.6c16c16c16c17p-10);
    p = hy_fma_sc(p, r, 0x1.1111111111111p-7);
    p = hy_fma_sc(p, r, 0x1.5555555555555p-5);
    p = hy_fma_sc(p, r, 0x1.5555555555555p-3);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    double res = ldexp(p, (int)kf);
    res = (x > 710.0) ? __builtin_inf() : res;
    res = (x < -746.0) ? 0.0 : res;
    return res;
}
)HIP";
    }
    if (pair_split) {
        // Exchange between the two lanes of a pair: DPP quad_perm [1,0,3,2] on the two halves of the double.
        src << R"HIP(
__device__ __forceinline__ double hy_swap1(double x)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
)HIP";
    }
    src << "__constant__ unsigned short hy_utbl[" << std::max<std::size_t>(utbl.size(), 1u) * L << "] = {";
    for (const auto &v : utbl) {
        for (const auto x : v) {
            if (x > 65535u) {
                why_not = "slot / variable index overflow in the lane tables";
                return;
            }
            src << x << ",";
        }
    }
    src << "};\n";
    {
        // Jet column of every state variable.
        std::vector<std::uint32_t> col_of(n_eq, 0);
        for_each_owner([&](auto &, auto &ow) {
            const auto &vv = utbl[ow.var_tbl];
            for (std::uint32_t l2 = 0; l2 < L && ow.mapped; ++l2) {
                if ((ow.valid_mask >> l2 & 1u) != 0u) {
                    col_of[vv[l2]] = utbl[ow.col_tbl][l2];
                }
            }
            for (std::uint32_t l2 = 0; l2 < ow.n_valid && !ow.mapped; ++l2) {
                col_of[vv[l2]] = ow.cbase + l2;
            }
        });
        if (m4) {
            // Source table of the cooperative store of the Taylor coefficients (mode 4): per stored row its index in a.tc
            // (variable * (order + 1) + k), the offset of its value for the first system of a wavefront inside the jets of
            // the wavefront, and the stride between the systems of the wavefront. Compact set (emitted_module::compact_tc):
            // a state variable defined by another state variable (x' = v) leaves with its order-0 row only.
            struct tc_entry {
                std::uint64_t row, off, stride;
            };
            std::vector<tc_entry> tc_src;
            if (one_lane) {
                // (Velocity-type jets [row][owner slot][system][lane]; current values of the derived variables behind them.)
                for_each_owner([&](auto &, auto &ow) {
                    const auto &vv = utbl[ow.var_tbl];
                    for (std::uint32_t l2 = 0; l2 < ow.n_valid; ++l2) {
                        const std::uint64_t var = vv[l2];
                        if (ow.derived) {
                            tc_src.push_back({var * (order + 1u), jet_rows_doubles + jet_off(ow) + l2, jet_sys(ow)});
                        } else {
                            for (std::uint32_t k = 0; k <= order; ++k) {
                                tc_src.push_back({var * (order + 1u) + k,
                                                  static_cast<std::uint64_t>(k) * spw * n_colp + jet_off(ow) + l2, jet_sys(ow)});
                            }
                        }
                    }
                });
            } else {
                for (std::uint32_t var = 0; var < n_eq; ++var) {
                    const bool derived = compact_tc && emit_detail::defined_by_state_variable(p, var);
                    for (std::uint32_t k = 0; k <= (derived ? 0u : order); ++k) {
                        tc_src.push_back({static_cast<std::uint64_t>(var) * (order + 1u) + k,
                                          static_cast<std::uint64_t>(k) * spw * n_colp + col_of[var], n_colp});
                    }
                }
            }
            if (n_tc_rows != tc_src.size()) {
                // (Two computations of one quantity: drift between them is a defect of the generator, not a refusal.)
                throw std::logic_error("mode 4: the source table of the Taylor coefficients has " + std::to_string(tc_src.size())
                                       + " rows, the LDS budget counted " + std::to_string(n_tc_rows));
            }
            src << "__constant__ unsigned long long hy_tc_src[" << std::max<std::size_t>(n_tc_rows, 1u) << "] = {";
            for (const auto &t : tc_src) {
                if (t.row >= (1ull << 20) || t.off >= (1ull << 20) || t.stride >= (1ull << 20)) {
                    why_not = "mode 4: index overflow in the source table of the Taylor coefficients";
                    return;
                }
                src << (t.row | (t.off << 20) | (t.stride << 40)) << "ull,";
            }
            src << "};\n";
        }
        src << "__constant__ unsigned short hy_col_of_var[" << n_eq << "] = {";
        for (const auto c : col_of) {
            src << c << ",";
        }
    }
    if (one_lane) {
        src << "};\n__constant__ double hy_rk[" << (order + 1u) << "] = {0.0,";
        for (std::uint32_t k = 1; k <= order; ++k) {
            src << fp_literal(1. / static_cast<double>(k)) << ",";
        }
    }
    src << "};\n__constant__ double hy_dtbl[" << std::max<std::size_t>(dtbl.size(), 1u) * L << "] = {";
    for (const auto &v : dtbl) {
        for (const auto x : v) {
            src << fp_literal(x) << ",";
        }
    }
    src << "};\n";
}

// Reads the layout and the tables; leaves the kernel head: LDS arrays, lane tables in registers, jet pointers.
void cluster2_gen::text_kernel_prologue()
{
    src << "extern \"C\" __global__ void __launch_bounds__(" << bs << ") hy_taylor(const hy_kargs a)\n{\n";
    src << "__shared__ " << (wide_rd ? "__attribute__((aligned(16))) " : "") << "double lds_slab["
        << lds_count("lds_slab") << "];\n";
    src << "const unsigned lane = threadIdx.x & 63u;\nconst unsigned wib = threadIdx.x >> 6;\n";
    src << "const unsigned l = lane % " << L << "u;\nconst unsigned q = lane / " << L << "u;\n";
    src << "const u64 N = a.N;\n";
    if (pair_split) {
        src << "const bool isB = (lane & 1u) != 0u;\nconst double fB = isB ? 1.0 : 0.0, fA = isB ? 0.0 : 1.0;\n";
    }
    src << "double *const slab = lds_slab + (wib * " << spw << "u + q) * " << slab_stride << "u;\n";
    if (one_lane) {
        if (bk_in_slab) {
            src << "double *const bk = slab + " << (slab_stride - 16u) << "u;\n";
        } else {
            src << "__shared__ double lds_bk[" << lds_count("lds_bk") << "];\ndouble *const bk = lds_bk + (wib * " << spw << "u + q) * 16u;\n";
        }
    }
    src << "const u64 gwave = (u64)blockIdx.x * " << wpb << "u + wib;\n";
    if (jet_lds) {
        src << "__shared__ double lds_jet[" << lds_count("lds_jet") << "];\n";
        src << "double *const jetw = lds_jet + wib * " << jet_doubles_per_wave << "u;\n";
        if (vexch) {
            // (The rows of the system of this lane: [system][column].)
            src << "const double *const jetq = jetw + q * " << n_col << "u;\n";
        }
        if (m4) {
            // Source table of the cooperative store of the Taylor coefficients: row | jet column << 16.
            src << "__shared__ unsigned long long lds_tcsrc[" << lds_count("lds_tcsrc") << "];\n";
            src << "for (unsigned i = threadIdx.x; i < " << n_tc_rows << "u; i += " << bs
                << "u) lds_tcsrc[i] = hy_tc_src[i];\n__syncthreads();\n";
        }
    } else {
        src << "double *const jetw = a.scratch + gwave * " << jet_doubles_per_wave << "ull;\n";
    }
    // The lane tables (state variable of every owner slot and lane) are read from LDS: in constant memory every lookup at
    // the pickup of a group and ahead of every store of its results is a vector load, and gfx9 counts loads and stores in
    // ONE in-order counter (vmcnt) - the address of each group of stores then waits for the acknowledgement of all the
    // stores before it (four owner slots: four round trips per group of systems; with the table in LDS: none).
    {
        const auto n_ut = lds_count("lds_utbl");
        src << "__shared__ unsigned short lds_utbl[" << n_ut << "];\n";
        src << "for (unsigned i = threadIdx.x; i < " << n_ut << "u; i += " << bs << "u) lds_utbl[i] = hy_utbl[i];\n";
        src << "__syncthreads();\n#define hy_utbl lds_utbl\n";
    }
    for (std::size_t t = 0; t < utbl.size(); ++t) {
        if (utexpr[t] == "ut" + std::to_string(t)) {
            src << "const unsigned ut" << t << " = hy_utbl[" << t * L << "u + l];\n";
        }
    }
    if (one_lane) {
        src << "__shared__ double lds_dt[" << lds_count("lds_dt") << "];\n";
        src << "for (unsigned i = threadIdx.x; i < " << dtbl.size() * L << "u; i += " << bs << "u) lds_dt[i] = hy_dtbl[i];\n";
        src << "__syncthreads();\nconst double *const dtl = lds_dt + l;\n";
        if (pp.rx[0] >= 0 && !fuse_rx) {
            src << "const double crs_r = hy_dtbl[" << st1.crs * L << "u + l];\n";
        }
    }
    if (!pk_tbl.empty()) {
        // (Factors of the packed evaluation: row 0 = ones - the series of a variable with a jet column -, row 1 = RN(1 / k).)
        src << "__shared__ double lds_fac[" << lds_count("lds_fac") << "];\n";
        src << "for (unsigned i = threadIdx.x; i < " << 2u * (order + 1u) << "u; i += " << bs << "u) lds_fac[i] = (i <= " << order
            << "u) ? 1.0 : hy_rk[i - " << (order + 1u) << "u];\n__syncthreads();\n";
    }
    for (std::size_t t = 0; !one_lane && t < dtbl.size(); ++t) {
        src << "const double dt" << t << " = hy_dtbl[" << t * L << "u + l];\n";
    }
    for (std::uint32_t x = 0; !pairk && x < n_cst; ++x) {
        src << "const double ccst" << x << " = dt" << cst_tbl[x] << ";\n";
    }
    for_each_owner([&](auto &gr, auto &ow) {
        if (ow.mapped) {
            // (Lane-reduced sums: the lane's jet column and whether the lane owns it come from the tables.)
            src << "const bool ovalid" << ow.col << " = ((" << ow.valid_mask << "u >> l) & 1u) != 0u;\n";
            const auto nm = (ow.derived ? "x0c" : "jc") + std::to_string(ow.col);
            src << "double *const " << nm << " = jetw + " << (ow.derived ? jet_rows_doubles : 0u) << "u + q * " << jet_sys(ow)
                << "u + hy_utbl[" << ow.col_tbl * L << "u + l];\n";
            src << "const double *const " << (ow.derived ? "x0r" : "jr") << ow.col << " = " << nm << ";\n";
            return;
        }
        src << "const bool ovalid" << ow.col << " = l < " << gr.n_valid << "u;\n";
        if (ow.derived) {
            // (Current values of the derived variables: after the jet rows of the wavefront. One pointer for
            // reading and writing: the idle lanes of a partially filled slot replicate the work of lane 0 bit by
            // bit and store the same values to the same entry.)
            src << "double *const x0c" << ow.col << " = jetw + " << jet_rows_doubles + jet_off(ow) << "u + q * " << jet_sys(ow)
                << "u + (ovalid" << ow.col << " ? l : 0u);\n";
            src << "const double *const x0r" << ow.col << " = x0c" << ow.col << ";\n";
            return;
        }
        if (one_lane) {
            src << "double *const jc" << ow.col << " = jetw + " << jet_off(ow) << "u + q * " << jet_sys(ow) << "u + (ovalid"
                << ow.col << " ? l : 0u);\n";
            src << "const double *const jr" << ow.col << " = jc" << ow.col << ";\n";
            return;
        }
        src << "double *const jc" << ow.col << " = jetw + q * " << n_colp << "u + (ovalid" << ow.col << " ? "
            << ow.cbase << "u + l : " << n_col << "u);\n";
        // The current state (order-0 row) is read from the column of the replicated variable by the idle lanes.
        src << "const double *const jr" << ow.col << " = jetw + q * " << n_colp << "u + " << ow.cbase
            << "u + (ovalid" << ow.col << " ? l : 0u);\n";
    });
    // Lane-reduced sums: the pointers of the packed final evaluation (pack_tail_slot()) are formed once here instead of in
    // every step - three table lookups in LDS and their address arithmetic per step; the registers are the ones the
    // operand table of the second round used to hold.
    for (const auto &[col, tb] : pk_tbl) {
        if (!lane_sum) {
            break;
        }
        for_each_owner([&, col = col, tb = tb](auto &, auto &ow) {
            if (ow.col == col) {
                src << "const double *const pk_jh" << col << " = jetw + q * " << jet_sys(ow) << "u + hy_utbl[" << tb[1] * L << "u + l];\n";
                src << "const double *const pk_fh" << col << " = lds_fac + hy_utbl[" << tb[2] * L << "u + l];\n";
                src << "double *const pk_v" << col << " = jetw + q * " << jet_sys(ow) << "u + hy_utbl[" << tb[0] * L << "u + l];\n";
            }
        });
    }
    // Lane slots of the final evaluation: slot h, lane l <-> jet column h * L + l (dummy column beyond the last one).
    for (std::uint32_t h = 0; !one_lane && h < n_hslots; ++h) {
        src << "double *const hc" << h << " = jetw + q * " << n_colp << "u + ((" << h * L << "u + l < " << n_col << "u) ? "
            << h * L << "u + l : " << n_col << "u);\n";
    }
}

// The event-equation section of mode 4. Reads opts.ev_prog, rounds and the jet layout; leaves ev_inline, ev_code, ev_coeffs,
// pe_lane_ev / pe_lane_sign and the per-lane offsets of the leaf positions in src.
void cluster2_gen::text_event_equations()
{
    // Event equations inside the stepper (emit_options::ev_prog; one-lane-per-pair kernel): their jets from the jets of the
    // state variables in LDS - every lane of a system runs the same statements; the terms of a sum of isomorphic terms
    // (a squared distance, a radial velocity) are evaluated side by side, term c by lane c (ev_lane_hooks) -, the three
    // norms extended to them, then the ordinary selector, final evaluation and state update of this kernel. What is left
    // to the kernels behind the stepper: event detection on a.ev_tc, times / outcomes / records (hy_ev_post). The
    // statements are generated here (their per-lane offsets are declared ahead of the work loop) and pasted into the tail.
    ev_inline = false;
    const bool packed_tail_ev = L >= 4u;
    if (m4 && one_lane && jet_lds && packed_tail_ev && opts.ev_prog != nullptr && !opts.exact_division && slab_stride >= n_own * L
        && opts.dev.events_in_stepper) {
        struct sv_loc {
            bool derived = false;
            std::uint64_t off = 0;
            std::uint32_t stride = 0;
            std::uint32_t parent = 0;
        };
        std::vector<sv_loc> loc(n_eq);
        for_each_owner([&](auto &gr, auto &ow) {
            const auto &vv = utbl[ow.var_tbl];
            for (std::uint32_t l2 = 0; l2 < ow.n_valid; ++l2) {
                auto &lc = loc[vv[l2]];
                lc.stride = jet_sys(ow);
                if (ow.derived) {
                    lc.derived = true;
                    lc.off = jet_rows_doubles + jet_off(ow) + l2;
                    for (const auto &o2 : gr.owners) {
                        if (o2.col == ow.parent) {
                            lc.parent = utbl[o2.var_tbl][l2];
                        }
                    }
                } else {
                    lc.off = jet_off(ow) + l2;
                }
            }
        });
        const auto rowst = static_cast<std::uint64_t>(spw) * n_colp;
        const std::function<std::string(std::uint32_t, std::uint32_t)> sv = [&](std::uint32_t i, std::uint32_t k) -> std::string {
            const auto &lc = loc[i];
            if (!lc.derived) {
                return "jetw[" + std::to_string(k * rowst + lc.off) + "u + q * " + std::to_string(lc.stride) + "u]";
            }
            if (k == 0u) {
                return "jetw[" + std::to_string(lc.off) + "u + q * " + std::to_string(lc.stride) + "u]";
            }
            // x^[k] = v^[k-1] * RN(1 / k): the rounded product the stepper itself would publish, kept out of contraction.
            const auto &pl_ = loc[lc.parent];
            return "hy_mul_nc(jetw[" + std::to_string((k - 1u) * rowst + pl_.off) + "u + q * " + std::to_string(pl_.stride) + "u], "
                   + fp_literal(1. / static_cast<double>(k)) + ")";
        };
        // (With the exclusion test below the jets of the event equations are stored behind it, and only by wavefronts in which
        // an event is possible: the detection kernel does not read the jets of the systems the test has ruled out.)
        const bool ev_store_late = true;
        const std::function<std::string(std::uint32_t, std::uint32_t, const std::string &)> ev_store
            = [&](std::uint32_t ev, std::uint32_t k, const std::string &v) {
                  if (ev_store_late) {
                      return std::string{};
                  }
                  return "a.ev_tc[(u64)" + std::to_string(static_cast<std::uint64_t>(ev) * (order + 1u) + k) + "u * N + s] = " + v + ";\n";
              };
        // Terms of a sum side by side on the lanes of the system: leaf position p of the shared shape is read at a per-lane
        // offset (evo<p>: the jet column, of the variable itself or - position-type variables - of the variable it is
        // derived from; evz<p>: the current value of a position-type variable).
        ev_lane_hooks hooks;
        hooks.max_terms = std::min<std::uint32_t>(4u, L);
        hooks.sv_class = [&](std::uint32_t i) { return loc[i].derived ? 1 : 0; };
        hooks.sv_lane = [&](std::uint32_t pp, std::uint32_t k, int cls) -> std::string {
            const auto ps = std::to_string(pp);
            if (cls == 0) {
                return "jetw[" + std::to_string(k * rowst) + "u + evo" + ps + "]";
            }
            if (k == 0u) {
                return "jetw[evz" + ps + "]";
            }
            return "hy_mul_nc(jetw[" + std::to_string((k - 1u) * rowst) + "u + evo" + ps + "], " + fp_literal(1. / static_cast<double>(k)) + ")";
        };
        hooks.lane_bcast = [&](const std::string &v, std::uint32_t c) {
            return "__shfl(" + v + ", (int)((threadIdx.x & " + std::to_string(64u - L) + "u) + " + std::to_string(c) + "u), 64)";
        };
        std::string why_ev;
        const bool use_lanes = true;
        // Close encounters: an event equation |r_i - r_j|^2 + c is, up to the constant, the squared distance whose Taylor
        // coefficients the lane of the pair (i, j) holds as the history of its pow recurrence (sB: b_k / b_0). Such events are
        // not evaluated at all: the lane of the pair contributes its history - one event per lane, every lane at the same
        // time (one exclusion test, one set of stores for ALL of them); order p, which the recursion of the state does not
        // need, costs one more convolution from the order-p coefficients of the positions.
        std::vector<char> ev_on_lane(opts.ev_prog->ev_u.size(), 0);
        if (pairk && ev_store_late && opts.dev.pair_events) {
            for (std::size_t ev = 0; ev < opts.ev_prog->ev_u.size(); ++ev) {
                pair_distance_event pe;
                const bool pe_ok = match_pair_distance_event(*opts.ev_prog, opts.ev_prog->ev_u[ev], pe);
                if (!pe_ok) {
                    continue;
                }
                const auto unordered = [](std::pair<std::uint32_t, std::uint32_t> x) {
                    return x.first < x.second ? x : std::pair<std::uint32_t, std::uint32_t>{x.second, x.first};
                };
                std::vector<std::pair<std::uint32_t, std::uint32_t>> want;
                for (const auto &d : pe.diffs) {
                    want.push_back(unordered(d));
                }
                std::sort(want.begin(), want.end());
                for (std::uint32_t cl = 0; cl < nc && cl < L; ++cl) {
                    std::vector<std::pair<std::uint32_t, std::uint32_t>> have;
                    for (std::uint32_t i = 0; i < 3u; ++i) {
                        have.push_back(unordered({pl.ext_u[cl][pp.de[i][0]], pl.ext_u[cl][pp.de[i][1]]}));
                    }
                    std::sort(have.begin(), have.end());
                    if (have == want && pe_lane_ev.count(cl) == 0u) {
                        pe_lane_ev[cl] = {static_cast<std::uint32_t>(ev), pe.c};
                        pe_lane_sign[cl] = pe.sign;
                        ev_on_lane[ev] = 1;
                        break;
                    }
                }
            }
        }
        const bool ev_ok = emit_event_jets_inline(*opts.ev_prog, opts, sv, ev_store, ev_code, ev_coeffs, why_ev,
                                                  use_lanes ? &hooks : nullptr, &ev_on_lane);
        if (!ev_ok) {
            pe_lane_ev.clear();
        }
        if (ev_ok) {
            ev_inline = true;
            // Per-lane offsets of the leaf positions (lanes beyond the last term replicate term 0).
            const auto pick = [&](const std::vector<std::uint64_t> &v) {
                std::string r = std::to_string(v[0]) + "u";
                for (std::size_t c = v.size(); c-- > 1u;) {
                    r = "(l == " + std::to_string(c) + "u ? " + std::to_string(v[c]) + "u : " + r + ")";
                }
                return r;
            };
            for (std::size_t pp = 0; use_lanes && pp < hooks.leaf_vars.size(); ++pp) {
                std::vector<std::uint64_t> off, str_, zoff, zstr;
                for (const auto var : hooks.leaf_vars[pp]) {
                    const auto &lc = loc[var];
                    const auto &src_ = lc.derived ? loc[lc.parent] : lc;
                    off.push_back(src_.off);
                    str_.push_back(src_.stride);
                    zoff.push_back(lc.off);
                    zstr.push_back(lc.stride);
                }
                src << "const unsigned evo" << pp << " = " << pick(off) << " + q * " << pick(str_) << ";\n";
                if (hooks.leaf_class[pp] == 1) {
                    src << "const unsigned evz" << pp << " = " << pick(zoff) << " + q * " << pick(zstr) << ";\n";
                }
            }
            if (!pe_lane_ev.empty()) {
                // Per lane: 1 / 0 (the pair of this lane has an event), the constant of the event equation, the row block of
                // the event in a.ev_tc (lanes without an event: a block of their own behind the last event).
                std::string on = "0.0", cst = "0.0", row = std::to_string(opts.ev_prog->ev_u.size()) + "u";
                for (const auto &[lane_, evc] : pe_lane_ev) {
                    const auto ls = "(l == " + std::to_string(lane_) + "u ? ";
                    // (The switch carries the sign of the squared distance in the event equation: +-1, 0 = no event.)
                    on = ls + (pe_lane_sign.at(lane_) < 0 ? "-1.0 : " : "1.0 : ") + on + ")";
                    cst = ls + fp_literal(evc.second) + " : " + cst + ")";
                    row = ls + std::to_string(evc.first) + "u : " + row + ")";
                }
                src << "const double pe_on = " << on << ";\nconst double pe_c = " << cst << ";\nconst u64 pe_row = (u64)" << row
                    << " * " << (order + 1u) << "u;\n";
            }
        }
    }
}

namespace
{

// (The plain-step text of a block is the ordinary one with a few statements exchanged: every exchange must find its place.)
std::string exchanged(std::string text, const std::string &from, const std::string &to)
{
    const auto pos = text.find(from);
    if (pos == std::string::npos || text.find(from, pos + 1u) != std::string::npos) {
        throw std::logic_error("hy_taylor (one lane per pair): the plain-step text does not find exactly one '" + from + "'");
    }
    return text.replace(pos, from.size(), to);
}

} // namespace

// Reads rounds and body; leaves the work loop up to and including the step body in src, bk_lds and plain_step.
void cluster2_gen::text_pickup()
{
    plain_step = one_lane && !m4 && jet_lds && !v5_flag("noplainstep");
    std::string work = R"HIP(
// Work distribution. Propagation (steps per system differ): a device-side queue, one group of systems at a time (taking
// chunks of 8 groups per atomic costs 1 % there: consecutive groups no longer run at the same time on neighbouring
// wavefronts, which is what lets the partial-line accesses to the SoA arrays meet in L2). Single steps (equal cost per
// group): a static interleaved schedule - group = iteration * wavefronts + wavefront - with the same locality and no
// atomics (a launch of 1 048 576 systems is 524 288 atomics on one address: 3 ms of a 6.5 ms launch).
const u64 hy_waves = (u64)gridDim.x * HY_WPB;
const bool hy_static = (HY_MODE != 1) && (HY_NO_STATIC == 0);
u64 hy_it = 0;
bool hy_queue_empty = false;
for (;;) {
u64 base = 0;
if (hy_static) {
    // (Exit decided per workgroup: the cooperative store of the Taylor coefficients below has workgroup barriers. A
    // wavefront beyond the end of the ensemble in a live workgroup replicates the last system, without side effects.)
    if (HY_M4 && (hy_it * (u64)gridDim.x + blockIdx.x) * (HY_WPB * SPW) >= N) break;
    base = (hy_it * hy_waves + gwave) * SPW;
    ++hy_it;
} else {
    if (lane == 0u) base = atomicAdd((u64 *)(a.counters + 2), (u64)SPW);
}
// NOTE: through readfirstlane the position is a scalar for the compiler and the exit of the work loop a wave-uniform
// branch (a shuffle / the wavefront index leave it "divergent": exec-mask bookkeeping around the whole step loop).
base = ((u64)__builtin_amdgcn_readfirstlane((unsigned)(base >> 32)) << 32) | (u64)__builtin_amdgcn_readfirstlane((unsigned)base);
if (!(HY_M4 && hy_static) && base >= N) break;
// NOTE: lanes beyond the end of the ensemble replicate the last system (no side effects).
bool live = (base + q) < N;
u64 s = live ? (base + q) : (N - 1u);
double t_hi = a.time_hi[s], t_lo = a.time_lo[s];
)HIP";
    if (plain_step) {
        // (The wavefront's number for the static schedule as a scalar: as a vector value it is live across the step loop,
        // whose two paths leave the allocator one register pair short - it then spills this one.)
        work = exchanged(work, "const u64 hy_waves = ", "const u64 hy_gwave = (u64)blockIdx.x * HY_WPB + (u64)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);\n"
                                                         "const u64 hy_waves = ");
        work = exchanged(work, "hy_waves + gwave) * SPW;", "hy_waves + hy_gwave) * SPW;");
    }
    src << work;
    for (std::uint32_t i = 0; i < p.n_par; ++i) {
        src << "const double par_" << i << " = a.pars[(u64)" << i << "u * N + s];\n";
    }
    for (const auto t : lane_par_tbls) {
        src << "const double lp" << t << " = a.pars[(u64)" << utname(t) << " * N + s];\n";
    }
    for_each_owner([&](auto &, auto &ow) {
        src << row0_w(ow) << " = a.state[(u64)hy_utbl[" << ow.var_tbl * L << "u + l] * N + s];\n";
    });
    src << "HY_WSYNC();\n" << (jet_lds ? "" : "__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, \"wavefront\");\n");
    std::string pickup = R"HIP(
hy_df tfin, rem;
tfin.hi = 0.0; tfin.lo = 0.0; rem.hi = 0.0; rem.lo = 0.0;
bool t_dir = true;
double mdt = __builtin_inf();
double step_lim = 0.0;
double thr = 0.0;
if (HY_MODE == 1) {
    tfin.hi = (a.tfin_hi != nullptr) ? a.tfin_hi[s] : a.tfin_s_hi;
    tfin.lo = (a.tfin_hi != nullptr) ? a.tfin_lo[s] : a.tfin_s_lo;
    hy_df tcur; tcur.hi = t_hi; tcur.lo = t_lo;
    rem = hy_df_sub(tfin, tcur);
    t_dir = (rem.hi > 0.0) || (rem.hi == 0.0 && rem.lo >= 0.0);
    if (a.lim != nullptr) mdt = a.lim[s];
    // (Propagation from grid point to grid point - hy_kargs::pad bit 2 in mode 1, emitted_module::grid_multi_step: the
    // system leaves the step loop after the first step which reaches a.tc_thr[s], with the coefficients of that step stored.)
    if ((a.pad & 4) != 0) thr = a.tc_thr[s];
} else {
    step_lim = a.lim[s];
    // (Taylor coefficients of a lock-step sweep on demand - hy_kargs::pad bit 2, the loop of propagate_grid() without a
    // callback: the NEXT GRID TIME of every system - a.tc_thr, or a.tfin_hi for callers of before round 6 -, and only the
    // steps which reach it store their coefficients - see emitted_module::tc_by_threshold.)
    if ((a.pad & 4) != 0) thr = (a.tc_thr != nullptr) ? a.tc_thr[s] : a.tfin_hi[s];
}
u64 n_steps = 0, iter = 0;
double min_h = __builtin_inf(), max_h = 0.0, last_h = 0.0;
i64 outcome = HY_OC_SUCCESS;
// NOTE: the step loop is left by the whole wavefront at once (wave-uniform exit): a system which has reached its final
// time keeps executing steps of length zero with all its bookkeeping frozen by selects (fin) until the other
// systems of the wavefront are done - a wavefront executes an iteration as long as one of its lanes is active
// anyway. With a per-lane exit the loop-carried values of the lanes which have left live across several
// hundred live registers of the remaining ones, which is where this toolchain's live-range splitting goes
// wrong (DESIGN.md, toolchain notes).
bool fin = false;
// (Did the system leave the step loop through a step clamped to its remaining time? hy_kargs::grid_done.)
bool gfin = false;
int nf_seen = 0;
// (Stepper with events which evaluates the event equations itself: does this system need its Taylor coefficients in
// memory? See "On-demand Taylor coefficients" below. hy_kargs::pad: bit 0 = store them for every system, bit 1 = store
// NOTHING but them - the regeneration launch on the snapshot of the state before the step.)
bool need_tc = true;
const bool hy_tc_only = HY_M4 && ((a.pad & 2) != 0);
)HIP";
    if (plain_step) {
        // (rlb = 0: the first step of a system is an ordinary one, which sets it.)
        pickup = exchanged(pickup, "hy_df tfin, rem;\ntfin.hi = 0.0; tfin.lo = 0.0; rem.hi = 0.0; rem.lo = 0.0;\n",
                           "hy_df tfin;\ntfin.hi = 0.0; tfin.lo = 0.0;\n// (A lower bound of the magnitude of the remaining time: see the plain step.)\n"
                           "double rlb = 0.0;\n");
        pickup = exchanged(pickup, "    rem = hy_df_sub(tfin, tcur);\n", "    const hy_df rem = hy_df_sub(tfin, tcur);\n");
    }
    src << pickup;
    // One-lane pair kernel: the per-system bookkeeping of the step loop (times, limits, counters, outcome: 30 registers
    // which nothing reads during the 20 orders) is parked in LDS between the tails of two steps - written at the end of
    // a tail, read back at the beginning of the next one - instead of being spilled to scratch by the register
    // allocator, whose reloads are scattered over the tail and each wait for a round trip through the vector memory
    // path. Every lane of a system holds the same values and stores them to the same address.
    bk_lds = one_lane;
    if (bk_lds) {
        bk_store();
        src << "HY_WSYNC();\n";
    }
    src << "for (;;) {\n";
    src << body;
}

// The step-size selector. Reads pe_lane_ev, the histories of the one-lane program, ev_code, rounds and pk_tbl; leaves the
// norms reduced over the lanes (with the event equations folded in), pe_g, tail_passes (with the jet reads issued ahead of
// the selector), kstride and the step size h.
void cluster2_gen::text_selector()
{
    // Close-encounter events on the lanes of their pairs (pe_lane_ev): g^[0] = b_0 + c, g^[k] = (b_k / b_0) b_0 from the
    // history of the pow recurrence, g^[p] from one more convolution; folded into the three norms of the lane BEFORE the
    // reduction over the lanes (masked: a lane without an event contributes nothing).
    if (!pe_lane_ev.empty()) {
        src << "HY_WSYNC();\n";
        std::string dK[3];
        for (std::uint32_t i = 0; i < 3u; ++i) {
            src << "const double pe_d" << i << " = " << slabk(order, utname(st1.s[i][0])) << " - " << slabk(order, utname(st1.s[i][1]))
                << ";\n";
            dK[i] = "pe_d" + std::to_string(i);
        }
        // b_p = 2 sum_i (sum_{j < p / 2} d_i[j] d_i[p - j] + 1/2 d_i[p / 2]^2)   (p even: src/detail/sum_sq.cpp:100-245)
        for (std::uint32_t i = 0; i < 3u; ++i) {
            src << "double pe_q" << i << " = " << dK[i] << " * " << sD[i][0] << ";\n";
            for (std::uint32_t j = 1; 2u * j < order; ++j) {
                src << "pe_q" << i << " = __builtin_fma(" << sD[i][j] << ", " << sD[i][order - j] << ", pe_q" << i << ");\n";
            }
            if (order % 2u == 0u) {
                src << "pe_q" << i << " = __builtin_fma(0.5 * " << sD[i][order / 2u] << ", " << sD[i][order / 2u] << ", pe_q" << i
                    << ");\n";
            }
        }
        src << "const double pe_bh = (pe_q0 + pe_q1) + pe_q2;\n";
        pe_g.resize(order + 1u);
        // (pe_on = +-1 on the lanes with an event: the sign of the squared distance in the event equation - exact. A lane
        // without an event gets zeros; it stores them into the spare block.)
        src << "const double pe_b0s = " << sB[0] << " * pe_on;\n";
        src << "const double pe_g0 = pe_b0s + pe_c;\n";
        pe_g[0] = "pe_g0";
        for (std::uint32_t k = 1; k < order; ++k) {
            src << "const double pe_g" << k << " = " << sB[k] << " * pe_b0s;\n";
            pe_g[k] = "pe_g" + std::to_string(k);
        }
        src << "const double pe_g" << order << " = (pe_bh + pe_bh) * pe_on;\n";
        pe_g[order] = "pe_g" + std::to_string(order);
        src << "m0 = hy_nmax(m0, fabs(pe_g0));\nmo = hy_nmax(mo, fabs(pe_g" << order
            << "));\nmom1 = hy_nmax(mom1, fabs(pe_g" << order - 1u << "));\n";
    }

    // Maximum over the lanes of the system: DPP stages where a DPP pattern yields an all-reduce step (xor 1, xor 2 within
    // quads; rotations by 4 and 8 within rows of 16 lanes once the quads are uniform), ds_bpermute for the others.
    // Packed tail (L >= 4): after the two stages inside the quads the three norms move to three lanes of every quad
    // (lane & 3 = 0: |x|, 1: |x^[p]|, 2 and 3: |x^[p-1]|) and the remaining stages reduce ONE value instead of three;
    // the logarithm of the selector is then evaluated once, on the packed lanes (hy_sel_log above).
    const bool packed_tail = L >= 4u;
    const auto red_ex = [&](std::uint32_t m, const char *v) -> std::string {
        if (m == 1u) {
            return std::string("hy_dpp<0xB1>(") + v + ")";
        }
        if (m == 2u) {
            return std::string("hy_dpp<0x4E>(") + v + ")";
        }
        if (m == 4u && L % 16u == 0u) {
            return std::string("hy_dpp<0x124>(") + v + ")";
        }
        if (m == 8u && L % 16u == 0u) {
            return std::string("hy_dpp<0x128>(") + v + ")";
        }
        return std::string("__shfl_xor(") + v + ", " + std::to_string(m) + ", 64)";
    };
    for (std::uint32_t m = 1; m < L; m *= 2u) {
        if (packed_tail && m == 4u) {
            break;
        }
        src << "m0 = hy_nmax(m0, " << red_ex(m, "m0") << ");\n";
        src << "mo = hy_nmax(mo, " << red_ex(m, "mo") << ");\n";
        src << "mom1 = hy_nmax(mom1, " << red_ex(m, "mom1") << ");\n";
    }
    if (packed_tail) {
        src << "const bool hy_q0 = (lane & 3u) == 0u, hy_q1 = (lane & 3u) == 1u;\n";
        src << "double nv = hy_q0 ? m0 : (hy_q1 ? mo : mom1);\n";
        for (std::uint32_t m = 4; m < L; m *= 2u) {
            src << "nv = hy_nmax(nv, " << red_ex(m, "nv") << ");\n";
        }
    }
    // Mode 4 (stepper with events): the norms over the state variables go to the kernel which extends them to the event
    // equations (hy_ev_jets). A wave-uniform branch; every lane of the system stores the same values.
    // (A separate specialisation of the kernel - opts.event_stepper - so that the propagation kernel is not touched: the
    // extra code, although never executed there, costs it spills in the step loop.)
    // Event equations inside the stepper: the statements prepared above (ev_code), then the three norms extended to them.
    if (ev_inline) {
        // (No scope around the statements: the coefficients of the event equations are read again by the exclusion test once
        // the step size is known. Their names live in a range of their own.)
        src << "double evm0 = 0.0, evmo = 0.0, evmom1 = 0.0;\n" << ev_code;
        for (const auto &c : ev_coeffs) {
            if (c.empty()) {
                continue;
            }
            src << "evm0 = hy_max(evm0, fabs(" << c[0] << "));\nevmo = hy_max(evmo, fabs(" << c[order]
                << "));\nevmom1 = hy_max(evmom1, fabs(" << c[order - 1u] << "));\n";
        }
        src << "nv = hy_nmax(nv, hy_q0 ? evm0 : (hy_q1 ? evmo : evmom1));\n";
        // (max |x_i| over the state variables and the event equations: the scale of the root finder's tolerance.)
        // (Not in the regeneration launch - hy_tc_only: it gets null pointers for everything but the coefficients.)
        src << "if (!hy_tc_only) a.max_abs_state[s] = hy_dpp<0x00>(nv);\n";
    }
    src << "#define HY_EV_INLINE " << (ev_inline ? 1 : 0) << "\n";
    src << "const bool nostate = " << ((m4 && !ev_inline) ? "true" : "false") << ";\n";
    // (The stepper with events never advances the time: hy_ev_post does, from the step size which was finally taken.)
    src << "const bool notime = " << (m4 ? "true" : "false") << ";\n";
    if (ev_inline) {
        // (Nothing to hand over: the norms are complete.)
    } else if (m4 && packed_tail) {
        // (Every lane stores: lane & 3 selects the row, the lanes of a system write identical values.)
        src << "a.sel_norms[(u64)(((lane & 3u) < 2u) ? (lane & 3u) : 2u) * N + s] = nv;\n";
    } else if (m4) {
        src << "a.sel_norms[s] = m0;\na.sel_norms[N + s] = mo;\na.sel_norms[2u * N + s] = mom1;\n";
    }
    // NOTE: rho = exp(log(x) / order) (hy_root): the minimum of the two estimates is taken on the exponents (exp is
    // monotone and keeps NaNs: the same selection as min(rho_o, rho_om1), src/taylor_02.cpp:1050-1072, one exp less).
    for_each_owner([&](auto &gr, auto &ow) {
        if (!one_lane || ow.derived) {
            return;
        }
        const owner_slot *dv = nullptr;
        for (const auto &o2 : gr.owners) {
            if (o2.derived && o2.parent == ow.col) {
                dv = &o2;
            }
        }
        tail_passes.push_back({&ow, dv, dv != nullptr && pk_tbl.count(ow.col) != 0u, {}, {}});
    });
    // (Doubles between two rows of a jet column.)
    kstride = static_cast<std::uint64_t>(spw) * n_colp;
    // The jet reads of the final evaluation (one-lane kernel, jets in LDS, compensated sums): issued HERE, ahead of the
    // selector's log / exp chain, which covers their latency - the history registers are dead in the tail, so the 20 rows
    // of a pass fit. "notailrd" among HEYOKA_AMD_V5_OPTS leaves them behind the step size, where the series consume them.
    if (one_lane && !m4 && jet_lds && opts.high_accuracy && packed_tail && !v5_flag("notailrd")) {
        src << "// (Jet reads of the final evaluation issued ahead of the selector.)\n";
        const auto hoist = [&](const std::string &ex) {
            auto nm = "trd" + std::to_string(n_trd++);
            src << "const double " << nm << " = " << ex << ";\n";
            return nm;
        };
        for (auto &tp : tail_passes) {
            const auto cs = std::to_string(tp.ow->col);
            if (tp.packed) {
                // (Row k of the lane's series at pk_jh[(k - 1) * stride], its factor at pk_fh[k]: see the pass below.)
                const auto &tb = pk_tbl.at(tp.ow->col);
                if (!lane_sum) {
                    src << "const double *const pk_jh" << cs << " = jetw + q * " << jet_sys(*tp.ow) << "u + hy_utbl[" << tb[1] * L << "u + l];\n";
                    src << "const double *const pk_fh" << cs << " = lds_fac + hy_utbl[" << tb[2] * L << "u + l];\n";
                }
                tp.rows.resize(order + 1u);
                tp.facs.resize(order + 1u);
                for (std::uint32_t k = 1; k <= order; ++k) {
                    tp.rows[k] = hoist("pk_jh" + cs + "[" + std::to_string((k - 1u) * kstride) + "]");
                    tp.facs[k] = hoist("pk_fh" + cs + "[" + std::to_string(k) + "]");
                }
            } else {
                for (std::uint32_t k = 0; k <= order; ++k) {
                    tp.rows.push_back(hoist("jr" + cs + "[" + std::to_string(k * kstride) + "]"));
                }
            }
        }
        src << "__builtin_amdgcn_sched_barrier(0);\n";
    }
    if (packed_tail) {
        // log(num / m) = log(num) - log(m): no quotients (0 -> +inf, inf -> -inf, inf - inf -> nan as for the quotient).
        src << "const double nw = (hy_q0 & (nv <= 1.0)) ? 1.0 : nv;\n";
        src << "const double lg = " << (sel_scalar ? "hy_sel_log_s" : "hy_sel_log") << "(nw);\n";
        src << "const double lg0 = hy_dpp<0x00>(lg), lg1 = hy_dpp<0x55>(lg), lg2 = hy_dpp<0xAA>(lg);\n";
        src << "const double lr_o = (lg0 - lg1) * " << fp_literal(1. / static_cast<double>(order)) << ";\n";
        src << "const double lr_om1 = (lg0 - lg2) * " << fp_literal(1. / static_cast<double>(order - 1u)) << ";\n";
        src << "const double rho_m = " << (sel_scalar ? "hy_sel_exp_s" : "exp") << "(hy_min(lr_o, lr_om1));\n";
    } else {
        src << "const double num_rho = (m0 <= 1.0) ? 1.0 : m0;\n";
        src << "const double lr_o = log(num_rho / mo) * " << fp_literal(1. / static_cast<double>(order)) << ";\n";
        src << "const double lr_om1 = log(num_rho / mom1) * " << fp_literal(1. / static_cast<double>(order - 1u)) << ";\n";
        src << "const double rho_m = exp(hy_min(lr_o, lr_om1));\n";
    }
    if (bk_lds) {
        bk_load();
    }
    // The limit of this step (remaining time / maximum step). NOTE: computed here, next to its only use, and not at the
    // top of the step: its inputs then do not have to be live (or reloaded) before the 20 orders.
    const std::string limit = R"HIP(
double lim;
if (HY_MODE == 1) {
    hy_df m; m.lo = 0.0;
    // NOTE: selects, not an if/else on the (per-lane) direction: see the note on HY_LIBM1.
    m.hi = t_dir ? mdt : -mdt;
    const bool lt_fwd = hy_df_lt(rem, m), lt_bwd = hy_df_lt(m, rem);
    const bool rem_first = (t_dir & lt_fwd) | (!t_dir & lt_bwd);
    lim = rem_first ? rem.hi : m.hi;
} else {
    lim = step_lim;
}
lim = fin ? 0.0 : lim;
)HIP";
    if (plain_step) {
        // The plain step. Almost every step of a propagation is one whose bookkeeping decides nothing: the selector's step
        // is far from the remaining time and from the maximum step, nobody finishes, the state stays finite. A wavefront all
        // of whose systems take such a step - one ballot, a wave-uniform branch - leaves out the limit, the remaining time
        // and every select which freezes a finished system. What a system must satisfy:
        //   - it is not finished, and this is not the last step its step limit allows;
        //   - 0 < h_sel and 2 h_sel <= min(rlb, mdt), where h_sel = rho_m * safety and rlb <= |remaining time| (below): the
        //     ordinary path then computes |lim| >= min(|rem.hi|, mdt) > h_sel, so h = +-h_sel, h != lim, h != rem.hi, the
        //     outcome is "success" and the step counts. (NaNs compare false: the ordinary path.)
        //   - its new time and state are finite (tested behind the series, as always: a wavefront which fails only there runs
        //     the ordinary bookkeeping with the same h).
        // The launch must be a propagation without grid flags and without Taylor coefficients on request (HY_PLAIN_STEP).
        // The ordinary path computes the remaining time rem = tfin - t exactly as it used to be carried (the same operation on
        // the same operands). Neither rem nor lim lives across the final evaluation: what the bookkeeping asks of them, h == lim
        // and h == rem.hi, is answered here (at_lim, at_rem: both false on a plain step).
        // rlb for the next step: the ordinary path leaves (|rem.hi| (1 - 2^-50) - |h|) (1 - 2^-50) - 2^-100 (|t| + |h|), a plain
        // step (rlb - |h|) (1 - 2^-50) - 2^-100 (|t| + |h|). The double-length sum t + h is within 2^-104 (|t| + |h|) of the exact
        // one and the factors absorb the roundings of these expressions, so rlb never exceeds the magnitude of the exact
        // tfin - t_new, whose computed high part is within 2^-52 of it; the factor 2 above leaves all that far behind. (A
        // remaining time which is a NaN, or points against the direction of the propagation, gives an rlb no step passes.)
        src << "#define HY_PLAIN_STEP ((HY_MODE == 1) & ((a.pad & 4) == 0) & (a.tc == nullptr))\n";
        src << "const double h_sel = rho_m * " << fp_literal(rhofac(order)) << ";\n";
        src << "const double h_two = h_sel + h_sel;\n";
        src << "const bool pl_no = fin | !((h_sel > 0.0) & (h_two <= rlb) & (h_two <= mdt)) | (iter + 1u == a.max_steps);\n";
        src << "double h;\nbool at_lim = false, at_rem = false;\n";
        src << "if (HY_PLAIN_STEP && __builtin_amdgcn_ballot_w64(pl_no) == 0ull) {\n"
               "h = t_dir ? h_sel : -h_sel;\n"
               "rlb = __builtin_fma(-0x1p-100, fabs(t_hi) + h_sel, (rlb - h_sel) * 0x1.ffffffffffff8p-1);\n} else {\n"
               "hy_df rem; rem.hi = 0.0; rem.lo = 0.0;\n";
        src << exchanged(limit, "double lim;\nif (HY_MODE == 1) {\n",
                         "double lim;\nif (HY_MODE == 1) {\n    hy_df tcur; tcur.hi = t_hi; tcur.lo = t_lo;\n    rem = hy_df_sub(tfin, tcur);\n");
        src << "h = hy_min(h_sel, fabs(lim));\nh = (lim < 0.0) ? -h : h;\nh = fin ? 0.0 : h;\n";
        src << "at_lim = (h == lim);\nat_rem = (h == rem.hi);\n";
        src << "rlb = __builtin_fma(-0x1p-100, fabs(t_hi) + fabs(h), (hy_min(t_dir ? rem.hi : -rem.hi, 0x1p+1000) * 0x1.ffffffffffff8p-1 - fabs(h))"
               " * 0x1.ffffffffffff8p-1);\n}\n";
        return;
    }
    src << limit;
    src << "double h = rho_m * " << fp_literal(rhofac(order)) << ";\n";
    src << "h = hy_min(h, fabs(lim));\nh = (lim < 0.0) ? -h : h;\n";
    // A system which is done takes steps of length EXACTLY zero (lim = 0 gives that unless the selector produced a nan):
    // the double-length time, the remaining time, the state and the step counters then reproduce themselves bit by bit,
    // and only the values which a zero-length step would overwrite need a select below (last_h, outcome).
    src << "h = fin ? 0.0 : h;\n";
}

// Reads ev_coeffs and pe_g; leaves the exclusion test and the stores of the event jets (event equations inside the stepper).
void cluster2_gen::text_event_exclusion()
{
    if (ev_inline) {
        // On-demand Taylor coefficients. Behind a step with events nothing reads the coefficients of the state variables
        // unless an event is detected (its callback may ask for dense output) or the caller asks for them. The stepper
        // runs the fast exclusion test of the detection (interval Horner enclosure of the event polynomial over the
        // step, src/detail/event_detection.cpp:704-816) on the jets it has just computed - CONSERVATIVELY: a system counts
        // as event-free only if the enclosure stays away from zero by 1e-8 of the largest intermediate magnitude, six
        // orders of magnitude above the rounding differences between this evaluation and the detection kernel's own -
        // and the workgroup stores its coefficients only if one of its systems may have an event. The integrator keeps
        // a snapshot of the state before the step: whoever reads coefficients which were not stored gets them from a
        // second launch on the snapshot (pad = 3), bit-identical.
        // First a cheaper bound which decides almost every system: |P(t) - c_0| <= sum_k |c_k| |h|^k on the step (20
        // multiply-adds per event equation); the interval enclosure (300 instructions per event equation) runs - behind a
        // wave-uniform branch - only in wavefronts where it leaves a system undecided.
        src << "bool maybe0 = false, pe_m0 = false;\n{\nconst double ah = fabs(h);\n";
        for (const auto &c : ev_coeffs) {
            if (c.empty()) {
                continue;
            }
            src << "{\ndouble r = fabs(" << c[order] << ");\n";
            for (std::uint32_t k = order - 1u; k >= 1u; --k) {
                src << "r = r * ah + fabs(" << c[k] << ");\n";
            }
            src << "r = r * ah;\nmaybe0 = maybe0 | !(fabs(" << c[0] << ") > r * 1.00000001);\n}\n";
        }
        // (The events on the lanes of their pairs: every lane tests ITS event - one instruction stream for all of them.)
        if (!pe_g.empty()) {
            src << "{\ndouble r = fabs(" << pe_g[order] << ");\n";
            for (std::uint32_t k = order - 1u; k >= 1u; --k) {
                src << "r = r * ah + fabs(" << pe_g[k] << ");\n";
            }
            src << "r = r * ah;\npe_m0 = (pe_on != 0.0) & !(fabs(" << pe_g[0] << ") > r * 1.00000001);\n}\n";
        }
        src << "}\nneed_tc = ((a.pad & 1) != 0);\nbool ev_possible = false;\n";
        // (Any lane of the system: one ballot, then the bits of the system's lanes.)
        const auto sys_any = [&](const char *v) {
            return "(((__builtin_amdgcn_ballot_w64(" + std::string(v) + ") >> ((threadIdx.x & 63u) & " + std::to_string(64u - L) + "u)) & "
                   + std::to_string((std::uint64_t(1) << L) - 1u) + "ull) != 0ull)";
        };
        src << "if (__builtin_amdgcn_ballot_w64(maybe0 | pe_m0) != 0ull) {\n";
        src << "bool maybe = false, maybe_te = false;\nconst double lo_h = (h < 0.0) ? h : 0.0, hi_h = (h < 0.0) ? 0.0 : h;\n";
        const auto enclosure = [&](const std::vector<std::string> &c) {
            src << "{\ndouble lo = " << c[order] << ", hi = lo, mm = fabs(lo);\n";
            for (std::uint32_t i = 1; i <= order; ++i) {
                src << "{\nconst double p0 = lo * lo_h, p1 = lo * hi_h, p2 = hi * lo_h, p3 = hi * hi_h;\n"
                    << "const double mn = fmin(fmin(p0, p1), fmin(p2, p3)), mx = fmax(fmax(p0, p1), fmax(p2, p3));\n"
                    << "lo = mn + " << c[order - i] << ";\nhi = mx + " << c[order - i] << ";\n"
                    << "mm = fmax(mm, fmax(fabs(lo), fabs(hi)));\n}\n";
            }
        };
        for (std::size_t ci = 0; ci < ev_coeffs.size(); ++ci) {
            const auto &c = ev_coeffs[ci];
            if (c.empty()) {
                continue;
            }
            enclosure(c);
            src << "const bool excl = (((lo > 0.0) & (hi > 0.0)) | ((lo < 0.0) & (hi < 0.0))) & (fmin(fabs(lo), fabs(hi)) > 1e-8 * mm);\n"
                << "maybe = maybe | !excl;\n" << (ci < opts.n_t_events ? "maybe_te = maybe_te | !excl;\n" : "") << "}\n";
        }
        src << "bool pe_m = false;\n";
        if (!pe_g.empty()) {
            enclosure(pe_g);
            src << "const bool excl = (((lo > 0.0) & (hi > 0.0)) | ((lo < 0.0) & (hi < 0.0))) & (fmin(fabs(lo), fabs(hi)) > 1e-8 * mm);\n"
                << "pe_m = pe_m0 & !excl;\n}\n";
        }
        // (The coefficients of the state variables are read behind the stepper only where a step may be TRUNCATED: at a
        // TERMINAL event: the events on the lanes of their pairs count as terminal whenever the integrator has one.)
        src << "ev_possible = (maybe & maybe0) | " << sys_any("pe_m") << ";\n";
        if (opts.n_t_events != 0u) {
            src << "need_tc = need_tc | (maybe_te & maybe0) | " << sys_any("pe_m") << ";\n";
        }
        src << "}\n";
        // (For the detection kernel: systems in which no event is possible are skipped without reading their event jets -
        // which are stored only by the wavefronts that hold such a system.)
        src << "if (!hy_tc_only) a.sel_norms[s] = ev_possible ? 1.0 : 0.0;\n";
        // (A caller who asked for the coefficients of every system - the raw stepper ABI, loops with dense output - gets the
        // event jets of every system as well.)
        src << "if (!hy_tc_only && (((a.pad & 1) != 0) | (__builtin_amdgcn_ballot_w64(ev_possible) != 0ull))) {\n";
        for (std::size_t ev = 0; ev < ev_coeffs.size(); ++ev) {
            for (std::uint32_t k = 0; !ev_coeffs[ev].empty() && k <= order; ++k) {
                src << "a.ev_tc[(u64)" << static_cast<std::uint64_t>(ev) * (order + 1u) + k << "u * N + s] = " << ev_coeffs[ev][k] << ";\n";
            }
        }
        // (The lanes of the pairs: every lane stores the row of ITS event - lanes without one into the spare block.)
        for (std::uint32_t k = 0; !pe_g.empty() && k <= order; ++k) {
            src << "a.ev_tc[(pe_row + " << k << "u) * N + s] = " << pe_g[k] << ";\n";
        }
        src << "}\n";
    }
}

// Reads tail_passes and rounds; leaves the final evaluation of the series, the new time, the Taylor coefficients on
// request, the state update and the bookkeeping of the step.
void cluster2_gen::text_final_evaluation_and_update()
{
    src << "asm volatile(\"\" ::: \"memory\");\n";
    // NOTE: with the jets in global scratch the lanes exchange them through memory: wavefront-scope fences.
    const char *jet_fence = jet_lds ? "" : "__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, \"wavefront\");\n";
    src << jet_fence;
    // Final evaluation of the Taylor series of the state variables (taylor_run_multihorner() / taylor_run_ceval(),
    // src/taylor_00.cpp:279-460). The jets live in LDS (or in the per-wave scratch), so the evaluation is spread
    // evenly over the lanes of the group: slot h, lane l <-> column h * L + l, ceil(n_eq / L) slots instead of
    // one per owner slot (3 instead of 4 for the 36 variables of the outer Solar System on 16 lanes).
    // (name of the new value, where the current value is read, where the new one goes)
    std::vector<std::tuple<std::string, std::string, std::string>> upd;
    // One pass per glue round: the variable with a jet column (v) and the one derived from it (x' = v), whose
    // coefficients are formed on the fly from the same column, x^[k] = v^[k-1] * RN(1 / k) - bit for bit the published
    // coefficient (ssa_emitter::div_const() in its reciprocal form). Both sums of a lane share the loads of the column
    // (one LDS read per order) and the powers of h; every pass is one instruction stream without selects.
    for (const auto &tp : tail_passes) {
        const auto &ow = *tp.ow;
        const auto *const dv = tp.dv;
        const auto xn = "xn" + std::to_string(ow.col);
        const auto xd = dv != nullptr ? "xn" + std::to_string(dv->col) : std::string{};
        const auto colp = "jr" + std::to_string(ow.col);
        if (tp.packed) {
            // A partially filled owner slot (18 velocity columns on 16 lanes leave 2): ONE series per lane - the
            // lanes [0, n) sum the velocity columns, the lanes [n, 2 n) the series derived from them, whose
            // coefficient k is row k - 1 of the same column times RN(1 / k); both kinds run the same statements, the
            // row shift sits in the lane's pointer and the factor (1 or RN(1 / k)) comes from a two-row table in LDS.
            // Six instructions per order instead of the ten of the two-series pass which 2 of 16 lanes used.
            const auto cs = std::to_string(ow.col);
            const auto &tb = pk_tbl.at(ow.col);
            // (The current value of the lane's variable: order-0 row of the column / entry of the derived variable.)
            if (!lane_sum) {
                src << "double *const pk_v" << cs << " = jetw + q * " << jet_sys(ow) << "u + hy_utbl[" << tb[0] * L << "u + l];\n";
            }
            src << "double " << xn << ";\n{\n";
            // (Row k of the lane's series at pk_j[(k - 1) * stride]: the velocity column from row 1 on, from row 0
            // on for the derived series.)
            if (tp.rows.empty()) {
                src << "const double *const pk_j = jetw + q * " << jet_sys(ow) << "u + hy_utbl[" << tb[1] * L << "u + l];\n";
                src << "const double *const pk_f = lds_fac + hy_utbl[" << tb[2] * L << "u + l];\n";
            }
            src << "double res = pk_v" << cs << "[0], comp = 0.0, cur_h = h;\n";
            for (std::uint32_t k = 1; k <= order; ++k) {
                src << "{\nconst double ck = " << tail_val(tp.rows, k, "pk_j[" + std::to_string((k - 1u) * kstride) + "]") << " * "
                    << tail_val(tp.facs, k, "pk_f[" + std::to_string(k) + "]") << ";\n"
                    << "const double tmp = ck * cur_h;\nconst double y = tmp - comp;\nconst double t = res + y;\n"
                    << "comp = (t - res) - y;\nres = t;\n";
                if (k < order) {
                    src << "cur_h = cur_h * h;\n";
                }
                src << "}\n";
            }
            src << xn << " = res;\n}\n";
            upd.emplace_back(xn, "pk_v" + cs + "[0]", "pk_v" + cs + "[0]");
            continue;
        }
        src << "double " << xn << ";\n";
        if (dv != nullptr) {
            src << "double " << xd << ";\n";
        }
        src << "{\n";
        if (opts.high_accuracy) {
            src << "double cprev = " << tail_val(tp.rows, 0, colp + "[0]") << ";\ndouble res = cprev, comp = 0.0, cur_h = h;\n";
            if (dv != nullptr) {
                src << "double resd = " << row0_r(*dv) << ", compd = 0.0;\n";
            }
            for (std::uint32_t k = 1; k <= order; ++k) {
                src << "{\nconst double ck = " << tail_val(tp.rows, k, colp + "[" + std::to_string(k * kstride) + "]") << ";\n";
                if (dv != nullptr) {
                    src << "const double cd = cprev * " << fp_literal(1. / static_cast<double>(k)) << ";\n"
                        << "const double tmpd = cd * cur_h;\nconst double yd = tmpd - compd;\n"
                        << "const double td = resd + yd;\ncompd = (td - resd) - yd;\nresd = td;\n";
                }
                src << "const double tmp = ck * cur_h;\nconst double y = tmp - comp;\nconst double t = res + y;\n"
                    << "comp = (t - res) - y;\nres = t;\ncprev = ck;\n";
                if (k < order) {
                    src << "cur_h = cur_h * h;\n";
                }
                src << "}\n";
            }
        } else {
            // Horner from the highest order down: the derived series needs the column shifted by one.
            src << "double res = " << colp << "[" << order * kstride << "];\n";
            if (dv != nullptr) {
                src << "double resd = " << colp << "[" << (order - 1u) * kstride << "] * "
                    << fp_literal(1. / static_cast<double>(order)) << ";\n";
            }
            for (std::uint32_t k = 1; k <= order; ++k) {
                const auto kk = order - k;
                src << "res = " << colp << "[" << kk * kstride << "] + res * h;\n";
            }
            if (dv != nullptr) {
                for (std::uint32_t k = 1; k <= order; ++k) {
                    const auto kk = order - k;
                    if (kk >= 1u) {
                        src << "resd = (" << colp << "[" << (kk - 1u) * kstride << "] * "
                            << fp_literal(1. / static_cast<double>(kk)) << ") + resd * h;\n";
                    } else {
                        src << "resd = " << row0_r(*dv) << " + resd * h;\n";
                    }
                }
            }
        }
        src << xn << " = res;\n";
        if (dv != nullptr) {
            src << xd << " = resd;\n";
        }
        src << "}\n";
        // (Event equations inside the stepper: the order-0 rows stay what they were - the Taylor coefficients
        // leave through the cooperative store behind the step - and the new state waits in the slab, which is
        // dead between the last order and the next step.)
        const auto new_at = [&](const owner_slot &o) {
            return ev_inline ? ("slab[" + std::to_string(o.col * L) + "u + l]") : row0_w(o);
        };
        upd.emplace_back(xn, row0_r(ow), new_at(ow));
        if (dv != nullptr) {
            upd.emplace_back(xd, row0_r(*dv), new_at(*dv));
        }
    }
    if (n_trd_used != n_trd) {
        // (Every read issued ahead of the selector must be the one its series consumes.)
        throw std::logic_error("hy_taylor (one lane per pair): " + std::to_string(n_trd - n_trd_used)
                               + " jet reads of the final evaluation were issued ahead of the selector and not consumed");
    }
    for (std::uint32_t c = 0; !one_lane && c < n_hslots; ++c) {
        upd.emplace_back("xn" + std::to_string(c), "hc" + std::to_string(c) + "[0]", "hc" + std::to_string(c) + "[0]");
        if (m4) {
            // (No state update in the stepper with events.)
            src << "const double xn" << c << " = hc" << c << "[0];\n";
            continue;
        }
        src << "double xn" << c << ";\n{\nconst double *c = hc" << c << ";\n";
        if (opts.high_accuracy) {
            src << "double res = c[0], comp = 0.0, cur_h = h;\n#pragma unroll\n";
            src << "for (unsigned k = 1; k <= " << order << "u; ++k) {\n";
            src << "const double tmp = c[(u64)k * " << kstride << "u] * cur_h;\nconst double y = tmp - comp;\n";
            src << "const double t = res + y;\ncomp = (t - res) - y;\nres = t;\ncur_h = cur_h * h;\n}\n";
        } else {
            src << "double res = c[(u64)" << order << "u * " << kstride << "u];\n#pragma unroll\n";
            src << "for (unsigned k = 1; k <= " << order << "u; ++k) {\n";
            src << "res = c[(u64)(" << order << "u - k) * " << kstride << "u] + res * h;\n}\n";
        }
        src << "xn" << c << " = res;\n}\n";
    }
    src << R"HIP(
double nt_hi, nt_lo;
{
    hy_df tcur; tcur.hi = t_hi; tcur.lo = t_lo;
    hy_df hh; hh.hi = h; hh.lo = 0.0;
    const hy_df nt = hy_df_add(tcur, hh);
    nt_hi = nt.hi; nt_lo = nt.lo;
}
int nfi = !(hy_finite(nt_hi) && hy_finite(nt_lo)) ? 1 : 0;
)HIP";
    for (const auto &u3 : upd) {
        // (The dummy column holds finite copies.)
        src << "nfi |= !hy_finite(" << std::get<0>(u3) << ") ? 1 : 0;\n";
    }
    // Any lane of the system: one ballot, then the bits of the system's lanes.
    // (Plain steps: only the ordinary path asks which system - below.)
    const auto nf_of_the_system = [&]() {
        src << "{\nconst u64 nfb = __builtin_amdgcn_ballot_w64(nfi != 0);\n";
        if (L == 64u) {
            src << "nfi = (nfb != 0ull) ? 1 : 0;\n}\n";
        } else {
            src << "nfi = (((nfb >> ((threadIdx.x & 63u) & " << (64u - L) << "u)) & " << ((std::uint64_t(1) << L) - 1u)
                << "ull) != 0ull) ? 1 : 0;\n}\n";
        }
    };
    if (!plain_step) {
        nf_of_the_system();
    }
    // Taylor coefficients on request (wave-uniform branch). NOTE: every lane stores: the idle lanes of a partially filled
    // owner slot replicate the variable of a valid lane and the lanes beyond the end of the ensemble replicate the
    // last system, so their stores write the same values to the same addresses - no divergent region in the step
    // loop (see the toolchain notes in DESIGN.md). A rolled loop with a running pointer: unrolled, the (order + 1)
    // store addresses per owner slot are invariants of the step loop and get hoisted into registers (84 x 64 bit for
    // the outer Solar System) for a path that only runs when the caller asks for the coefficients.
    if (one_lane && jet_lds && !m4) {
        // (A zero-length step - a system which has reached its last grid point - stores like the reference's lock-step
        // loop does; a non-finite new time compares false and stores nothing: nobody reads those coefficients.)
        // A step clamped to its limit stores as well: the last step of a lane ends at tlast - rem.lo, whose high part can
        // land on either side of the last grid time (grids ending at 0, crossing 0, backward runs to 0) while hy_grid_post
        // (h == rem.hi) evaluates every remaining grid point from these coefficients. (Steps clamped by max_delta_t store
        // needlessly: harmless.)
        src << "const bool hy_reach = (h > 0.0) ? (nt_hi >= thr) : (nt_hi <= thr);\n";
        // (fin: a system which left the step loop in an EARLIER iteration idles with zero-length steps until its wavefront is
        // done or its slot is refilled - in a launch from grid point to grid point those must not overwrite the coefficients
        // of its exit step.)
        src << "const bool tc_sys = ((a.pad & 4) == 0) | (!fin & ((h == 0.0) | " << (plain_step ? "at_lim" : "(h == lim)") << " | hy_reach));\n";
        src << "if (a.tc != nullptr && tc_sys) {\n";
    } else {
        src << (jet_lds ? "if (a.tc != nullptr && !HY_M4) {\n" : "if (a.tc != nullptr) {\n");
    }
    for_each_owner([&](auto &, auto &ow) {
        if (ow.derived) {
            src << "{\nconst double *c = jr" << ow.parent << ";\ndouble *tcp = a.tc + ((u64)hy_utbl[" << ow.var_tbl * L
                << "u + l] * " << (order + 1u) << "u) * N + s;\n*tcp = " << row0_r(ow) << ";\ntcp += N;\n"
                << "#pragma nounroll\nfor (unsigned k = 1; k <= " << order << "u; ++k) {\n*tcp = c[(u64)(k - 1u) * "
                << kstride << "u] * hy_rk[k];\ntcp += N;\n}\n}\n";
            return;
        }
        src << "{\nconst double *c = jr" << ow.col << ";\ndouble *tcp = a.tc + ((u64)hy_utbl[" << ow.var_tbl * L
            << "u + l] * " << (order + 1u) << "u) * N + s;\n"
            << "#pragma nounroll\nfor (unsigned k = 0; k <= " << order << "u; ++k) {\n*tcp = c[(u64)k * "
            << kstride << "u];\ntcp += N;\n}\n}\n";
    });
    src << "}\n";
    // The new state becomes the order-0 row of the jets (read back by the owner lanes at the top of the next step).
    src << "HY_WSYNC();\n" << jet_fence;
    if (plain_step) {
        // The plain step (see text_selector()): what the ordinary bookkeeping below leaves for a system which is not finished,
        // takes h = +-h_sel != lim, rem.hi and stays finite, without its selects; back to the parked record go the words this
        // changes. The ordinary path follows as the other branch, up to the stores of the record in text_refill_and_tail().
        src << "if (HY_PLAIN_STEP && __builtin_amdgcn_ballot_w64(pl_no | (nfi != 0)) == 0ull) {\n";
        for (const auto &u3 : upd) {
            src << std::get<2>(u3) << " = " << std::get<0>(u3) << ";\n";
        }
        src << "HY_WSYNC();\n" << jet_fence;
        src << R"HIP(
{
    const double ah = fabs(h);
    t_hi = nt_hi;
    t_lo = nt_lo;
    last_h = h;
    outcome = HY_OC_SUCCESS;
    n_steps = n_steps + 1u;
    iter = iter + 1u;
    min_h = hy_min(min_h, ah);
    max_h = hy_max(max_h, ah);
}
)HIP";
        bk_store(3);
        src << "} else {\n";
        nf_of_the_system();
    }
    for (const auto &u3 : upd) {
        // (A zero-length step leaves the state untouched bit by bit: x + 0 * ... = x also in the compensated sum.)
        src << std::get<2>(u3) << " = (fin | nostate) ? " << std::get<1>(u3) << " : " << std::get<0>(u3) << ";\n";
    }
    src << "HY_WSYNC();\n" << jet_fence;
    std::string ordinary = R"HIP(
{
    // Bookkeeping of the reference's step() / propagate_until() loops (src/taylor_adaptive_batch.cpp:632-727,
    // :1395-1520) on values frozen once the system is done.
    const bool nf = nfi != 0;
    const i64 oc_new = nf ? HY_OC_ERR_NF_STATE : ((h == lim) ? HY_OC_TIME_LIMIT : HY_OC_SUCCESS);
    bool done = nf | (HY_MODE != 1);
    const u64 ns_new = n_steps + ((!done & (h != 0.0)) ? 1u : 0u);
    const bool upd = !done & (oc_new == HY_OC_SUCCESS);
    const double ah = fabs(h);
    const double mn_new = upd ? hy_min(min_h, ah) : min_h;
    const double mx_new = upd ? hy_max(max_h, ah) : max_h;
    done |= (h == rem.hi);
    gfin = fin ? gfin : (h == rem.hi);
    done |= HY_GRID_STOP;
    hy_df tnew; tnew.hi = nt_hi; tnew.lo = nt_lo;
    const hy_df rem_new = hy_df_sub(tfin, tnew);
    const u64 it_new = iter + 1u;
    const bool sl = !done & (it_new == a.max_steps);
    const i64 oc_fin = sl ? HY_OC_STEP_LIMIT : oc_new;
    done |= sl;
    nf_seen |= (!fin & nf & !nostate) ? 1 : 0;
    // (fin: h = 0, hence nt = t, rem_new = rem, ns_new = n_steps, no min / max update - see above.)
    t_hi = notime ? t_hi : nt_hi;
    t_lo = notime ? t_lo : nt_lo;
    last_h = fin ? last_h : h;
    outcome = fin ? outcome : oc_fin;
    n_steps = ns_new;
    min_h = mn_new;
    max_h = mx_new;
    rem.hi = rem_new.hi;
    rem.lo = rem_new.lo;
    iter = it_new;
    fin = fin | done;
}
)HIP";
    if (plain_step) {
        // (The remaining time of this step was computed next to its limit, in text_selector(), with the two comparisons; none
        // is carried.)
        ordinary = exchanged(ordinary, "    hy_df tnew; tnew.hi = nt_hi; tnew.lo = nt_lo;\n    const hy_df rem_new = hy_df_sub(tfin, tnew);\n", "");
        ordinary = exchanged(ordinary, "hence nt = t, rem_new = rem, ns_new", "hence nt = t, ns_new");
        ordinary = exchanged(ordinary, "    rem.hi = rem_new.hi;\n    rem.lo = rem_new.lo;\n", "");
        ordinary = exchanged(ordinary, "((h == lim) ? HY_OC_TIME_LIMIT", "(at_lim ? HY_OC_TIME_LIMIT");
        ordinary = exchanged(ordinary, "    done |= (h == rem.hi);\n    gfin = fin ? gfin : (h == rem.hi);\n", "    done |= at_rem;\n    gfin = fin ? gfin : at_rem;\n");
    }
    src << ordinary;
}

// Reads rounds and the variant; leaves the per-system refill, the end of the step loop, the cooperative store of mode 4
// and the final stores of a group of systems.
void cluster2_gen::text_refill_and_tail()
{
    // Per-system refill (propagations through the device-side work queue): the step loop is left by the whole wavefront at
    // once, so a system which reaches its final time early idles - zero-length steps - until the slowest of the SPW
    // systems of its wavefront is done. With heterogeneous step counts (per-lane final times T * U(0.5, 1.5): 37 .. 127 steps
    // per system) that costs E[max of 4] / mean = 1.3x: 0.78 of the rate of a uniform ensemble (bench.py, divergence leg).
    // Here a finished system is retired on the spot - its results stored like at the end of the kernel - and its lanes pull
    // the next system from the queue: one atomic per system instead of one per wavefront, only behind a wave-uniform test
    // that some system of the wavefront has just finished. (The reference's lanes idle like the old loop:
    // src/taylor_adaptive_batch.cpp:1378-1460.)
    const bool refill = one_lane && !m4 && jet_lds && p.n_par == 0u && lane_par_tbls.empty() && L < 64u
                        && opts.dev.refill;
    if (refill) {
        src << "if (!hy_static && !hy_queue_empty && __builtin_amdgcn_ballot_w64(fin) != 0ull) {\n";
        // 1. Retire.
        for_each_owner([&](auto &, auto &ow) {
            src << "if (fin && ovalid" << ow.col << " && live) a.state[(u64)hy_utbl[" << ow.var_tbl * L
                << "u + l] * N + s] = " << row0_w(ow) << ";\n";
        });
        src << R"HIP(
if (fin && l == 0u && live) {
    a.time_hi[s] = t_hi;
    a.time_lo[s] = t_lo;
    a.last_h[s] = last_h;
    a.outcome[s] = outcome;
    a.min_h[s] = min_h;
    a.max_h[s] = max_h;
    a.n_steps[s] = n_steps;
    if (HY_GRID_FLAGS) a.grid_done[s] = gfin ? 1.0 : 0.0;
    if (nf_seen != 0) atomicAdd(a.counters, 1u);
}
// 2. The next system of the queue, for every finished system of the wavefront (its lane 0 asks, the others listen).
u64 snew = 0;
if (fin && l == 0u) snew = atomicAdd((u64 *)(a.counters + 2), (u64)1);
{
    const int src_lane = (int)((threadIdx.x & 63u) - l);
    const unsigned lo_ = (unsigned)__shfl((int)(unsigned)snew, src_lane, 64);
    const unsigned hi_ = (unsigned)__shfl((int)(unsigned)(snew >> 32), src_lane, 64);
    snew = ((u64)hi_ << 32) | (u64)lo_;
}
const bool got = fin && (snew < N);
// (The queue position only grows: one request beyond the end means that the queue is empty - stop asking.)
if (__builtin_amdgcn_ballot_w64(fin && !got) != 0ull) hy_queue_empty = true;
live = fin ? got : live;
nf_seen = fin ? 0 : nf_seen;
s = got ? snew : s;
// 3. Its state, times and limits; a fresh set of counters.
if (got) {
    t_hi = a.time_hi[s];
    t_lo = a.time_lo[s];
)HIP";
        for_each_owner([&](auto &, auto &ow) {
            src << row0_w(ow) << " = a.state[(u64)hy_utbl[" << ow.var_tbl * L << "u + l] * N + s];\n";
        });
        std::string fresh = R"HIP(
    tfin.hi = (a.tfin_hi != nullptr) ? a.tfin_hi[s] : a.tfin_s_hi;
    tfin.lo = (a.tfin_hi != nullptr) ? a.tfin_lo[s] : a.tfin_s_lo;
    hy_df tcur; tcur.hi = t_hi; tcur.lo = t_lo;
    rem = hy_df_sub(tfin, tcur);
    t_dir = (rem.hi > 0.0) || (rem.hi == 0.0 && rem.lo >= 0.0);
    mdt = (a.lim != nullptr) ? a.lim[s] : __builtin_inf();
    thr = ((a.pad & 4) != 0) ? a.tc_thr[s] : 0.0;
    n_steps = 0;
    iter = 0;
    min_h = __builtin_inf();
    max_h = 0.0;
    last_h = 0.0;
    outcome = HY_OC_SUCCESS;
    fin = false;
    gfin = false;
}
HY_WSYNC();
)HIP";
        if (plain_step) {
            // (The first step of the new system is an ordinary one.)
            fresh = exchanged(fresh, "    rem = hy_df_sub(tfin, tcur);\n", "    const hy_df rem = hy_df_sub(tfin, tcur);\n    rlb = 0.0;\n");
        }
        src << fresh;
        if (bk_lds) {
            bk_store(2);
        }
        src << "}\n";
    }
    if (bk_lds) {
        bk_store(1);
    }
    if (plain_step) {
        // (The end of the ordinary path: text_final_evaluation_and_update().)
        src << "}\n";
    }
    src << R"HIP(
if (__builtin_amdgcn_ballot_w64(!fin) == 0ull) break;
}
if (nf_seen != 0 && l == 0u && live) atomicAdd(a.counters, 1u);
)HIP";
    if (jet_lds && m4) {
        // Mode 4: the Taylor coefficients of the workgroup's systems (consecutive under the static schedule) leave through
        // a cooperative store - [variable][order] rows of HY_WPB * SPW consecutive systems, whole 128-byte lines for the
        // 16 systems of the lane-pair kernel - instead of 16-byte pieces per wavefront (the per-wavefront stores make
        // the 1 048 576-system stepper with events transaction bound: 8 ms instead of 3).
        const auto spb = wpb * spw;
        // NOTE: the (row, source offset, stride) of every stored row comes from a table in LDS (lds_tcsrc, filled once per
        // workgroup from hy_tc_src): with the table in global / constant memory every iteration of this loop issues vector
        // loads BEHIND the stores of the previous one, and gfx9 counts loads and stores in one in-order counter (vmcnt) -
        // each iteration then waits for a store acknowledgement (12 iterations: 6 us per group of systems, 1.5 ms of a
        // 4.2 ms launch on 1 048 576 systems).
        // (Event equations inside the stepper: only if one of the systems of the workgroup needs them - need_tc.)
        src << "{\nconst int hy_wg_tc = __syncthreads_or(need_tc ? 1 : 0);\n";
        src << "if (hy_wg_tc == 0 && threadIdx.x == 0u) atomicAdd(a.counters + 4, 1u);\n";
        src << "if (hy_wg_tc != 0) {\n";
        src << "const u64 bs0 = base - (u64)wib * SPW;\n";
        src << "for (unsigned idx = threadIdx.x; idx < " << n_tc_rows * spb << "u; idx += " << bs << "u) {\n";
        src << "const unsigned sy = idx % " << spb << "u;\nconst unsigned long long te = lds_tcsrc[idx / " << spb << "u];\n";
        src << "const unsigned row = (unsigned)(te & 0xfffffull), off = (unsigned)((te >> 20) & 0xfffffull), sst = "
               "(unsigned)(te >> 40);\n";
        src << "const u64 sg = bs0 + sy;\n";
        src << "const double val = lds_jet[(sy / SPW) * " << jet_doubles_per_wave << "u + off + (sy % SPW) * sst];\n";
        src << "if (sg < N) a.tc[(u64)row * N + sg] = val;\n}\n}\n__syncthreads();\n}\n";
    }
    src << R"HIP(
)HIP";
    for_each_owner([&](auto &, auto &ow) {
        if (m4 && !ev_inline) {
            // (The stepper with events leaves the state, the time and the step size to the kernels behind it -
            // unless it evaluates the event equations itself: then the state is final here.)
            return;
        }
        src << "if (ovalid" << ow.col << " && live && !hy_tc_only) a.state[(u64)hy_utbl[" << ow.var_tbl * L << "u + l] * N + s] = "
            << (ev_inline ? ("slab[" + std::to_string(ow.col * L) + "u + l]") : row0_w(ow)) << ";\n";
    });
    src << R"HIP(
if (l == 0u && live && !hy_tc_only) {
    if (!HY_M4) {
        if (HY_MODE != 2) {
            a.time_hi[s] = t_hi;
            a.time_lo[s] = t_lo;
        } else {
            const_cast<double *>(a.lim)[s] = last_h;
        }
    }
    if (!HY_M4 || HY_EV_INLINE) a.last_h[s] = last_h;
    a.outcome[s] = outcome;
    if (HY_MODE == 1) {
        a.min_h[s] = min_h;
        a.max_h[s] = max_h;
        a.n_steps[s] = n_steps;
        if (HY_GRID_FLAGS) a.grid_done[s] = gfin ? 1.0 : 0.0;
    }
}
}
}
)HIP";
}

// Leaves the emitted_module and the typed verdict in res.
void cluster2_gen::finish()
{
    res.mod.source = src.str();
    res.mod.kernel_name = "hy_taylor";
    res.mod.dout_name = "hy_dout";
    res.mod.block_size = bs;
    res.mod.lanes_per_system = L;
    res.mod.lds_bytes = 0;
    res.mod.mode = emit_mode::cluster;
    res.mod.n_statements = e.n_stmt;
    res.mod.scratch_per_wave = jet_lds ? 0u : jet_doubles_per_wave;
    res.mod.persistent = true;
    if (pairk) {
        // NOTE: MachineLICM hoists the materialisation of ~50 fp64 literals (1 / k, the polynomial constants of the
        // step-size selector) out of the step loop into SGPR pairs: pointers and masks are then spilled to VGPR lanes and
        // come back through 186 v_readlane_b32 per step (VALU issue slots). Without it: 20, and 7 % fewer VALU
        // instructions in the loop (measured: +2 % system-steps/s, profiles/experiments/run17.sh).
        res.mod.compile_flags = "-mllvm -disable-machine-licm";
        if (one_lane) {
            // NOTE: no merging of LDS accesses: on gfx950 a ds_read2_b64 is serviced at half the rate of two ds_read_b64
            // (8 against 2 x 2 LDS cycles per wavefront) and this kernel is within 25 % of the LDS throughput.
            res.mod.compile_flags += " -Xclang -target-feature -Xclang -load-store-opt -mllvm -amdgpu-load-store-vectorizer=0";
        }
    }
    res.mod.tc_optional = true;
    res.mod.cluster_mode4 = m4;
    res.mod.events_in_stepper = ev_inline;
    res.mod.compact_tc = compact_tc;
    res.mod.tc_by_threshold = one_lane && jet_lds && !m4;
    res.mod.grid_multi_step = res.mod.tc_by_threshold;
    res.jets_in_lds = one_lane && jet_lds;
    res.variant = variant;
    res.mod.cluster_generation = one_lane ? 5 : (pair_split ? 3 : 2);
    res.mod.notes = std::string(one_lane ? "cluster mode v5 (one lane per pair, 2 wavefronts per SIMD): "
                                     : (pair_split ? "cluster mode v3 (lane pairs, 2 wavefronts per SIMD): " : "cluster mode v2 (pipelined): "))
                + std::to_string(nc) + " clusters of " + std::to_string(t0().size())
                + " nodes, L=" + std::to_string(L) + ", " + std::to_string(pl.n_slots) + " LDS slots x2, "
                + std::to_string(n_own) + " state-variable owner slots, " + std::to_string(utbl.size())
                + " slot tables, jets in " + (jet_lds ? "LDS" : "global scratch")
                + (one_lane ? ", slab layout: " + std::to_string(bank_cost) + " conflict cycles per step in the model" : std::string{})
                + (lane_sum ? ", later sums reduced across the lanes of the first round" : "")
                + (plain_step ? ", plain steps leave out the bookkeeping of the step loop" : "")
                + (ev_inline ? "; event equations, final step size and state update inside the stepper" : "");
}

} // namespace heyoka_amd::cluster2_detail
namespace heyoka_amd
{

emitted_module emit_cluster_v2(const taylor_program &p, const emit_options &opts, emit_refusal &why_not)
{
    // The one-lane pair kernel first (pair-pattern systems without runtime parameters, not the stepper with events); if
    // its shape requirements fail or the jets of its systems do not fit in LDS, the lane-pair / pipelined kernels.
    // Few pairs (3 or 6: model::nbody(3), (4)): with 4 / 8 lanes per system a CU holds 128 / 64 systems, whose jets do not
    // fit in its LDS - and the lane-pair kernel with the jets in global scratch which used to serve them spills 176 / 116
    // registers. More lanes per system than pairs (idle lanes replicate pair 0 and write to dummy slots, like the 16th lane
    // of the outer Solar System) bring the systems per CU down to what fits: the second and third attempts.
    emit_refusal why1;
    const bool try_one_lane = opts.cluster_kernel == 0 || opts.cluster_kernel == 5;
    for (const std::uint32_t min_lanes : {4u, 8u, 16u}) {
        why1.clear();
        auto at = cluster2_detail::cluster2_gen(p, opts, why1, try_one_lane, min_lanes).run();
        const bool is_v5 = why1.empty() && at.variant == cluster2_detail::cluster2_variant::one_lane, in_lds = at.jets_in_lds;
        if (try_one_lane) {
            detail::log_message(log_level::debug, "one-lane-per-pair kernel, at least " + std::to_string(min_lanes) + " lanes per system: "
                                              + (!why1.empty() ? why1.text : (!is_v5 ? "not applicable" : (in_lds ? "accepted" : "the jets of the systems of a CU do not fit in its LDS"))));
        }
        if (why1.empty() && (in_lds || !is_v5)) {
            why_not.clear();
            return std::move(at.mod);
        }
        // (Another attempt only for the reasons which more lanes per system cure.)
        if (!try_one_lane || (!why1.empty() && !at.more_lanes_cure) || (why1.empty() && !is_v5)) {
            break;
        }
    }
    return cluster2_detail::cluster2_gen(p, opts, why_not, false, 4u).run().mod;
}

} // namespace heyoka_amd
