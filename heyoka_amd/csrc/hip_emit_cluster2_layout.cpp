// Cluster code generation, version 2 (hip_emit_cluster2_gen.hpp): the consumer-arranged slab slots of the one-lane-per-pair
// kernel - the part of stage 1 which layout_one_lane() calls - and the helpers of the lane tables.
#include <algorithm>
#include <cstdio>
#include <functional>

#include "hip_emit_cluster2_gen.hpp"

namespace heyoka_amd::cluster2_detail
{

// The consumer-arranged slots (wide_rd). Reads the wide-read analysis, att, vexch and bk_in_slab; leaves wide_pr / wide_rx,
// slab_stride_opt, bank_cost, pl.slot_of and pl.n_slots - or wide_rd = false where the stores cannot be arranged.
void cluster2_gen::place_wide_read_slots()
{
    const auto W = (n_args + 2u) & ~1u; // slots of an operand array (>= one spare slot, even)
    const auto nb = static_cast<std::uint32_t>(bodies.size());
    const auto &grp = pl.groups[0];
    // Address lists of the LDS instructions of a round (doubles, relative to the slab of the system), per lane of a
    // system; filled for a given layout by addr_lists().
    struct lds_op {
        int width; // 16: ds_read_b128, 8: ds_read_b64, -8: ds_write_b64
        std::vector<std::uint32_t> addr;
    };
    // (Velocity exchange: no position slots.)
    const auto pos_sz = vexch ? 0u : 4u * nb;
    std::uint32_t Dd = W * n_rank, pos_base = 0, op_base = pos_sz;
    // Position of operand a of the sums of rank r inside a coordinate block: arr_pos[r][a]. Default: arrays of W slots
    // one after the other; replaced below by a placement without store conflicts where one exists.
    std::vector<std::vector<std::uint32_t>> arr_pos(n_rank, std::vector<std::uint32_t>(n_args));
    for (std::uint32_t r = 0; r < n_rank; ++r) {
        for (std::uint32_t a = 0; a < n_args; ++a) {
            arr_pos[r][a] = W * r + a;
        }
    }
    std::uint32_t dummy_pos[2] = {W - 1u, 2u * W - 1u}; // (spare slots of the arrays of rank 0 / rank 1)
    std::uint32_t blk_used = W * n_rank;                 // (slots of a coordinate block)
    const auto op_slot = [&](std::uint32_t coord, std::uint32_t rank, std::uint32_t a) {
        return op_base + Dd * coord + arr_pos[rank][a];
    };
    // (Dummy slots of the idle lanes: the spare slot of the arrays of rank 0 (products) and rank 1 (reactions).)
    const auto dummy_pr = [&](std::uint32_t i) { return op_base + Dd * i + dummy_pos[0]; };
    const auto dummy_rx = [&](std::uint32_t i) { return op_base + Dd * i + dummy_pos[1]; };
    // Which operand position reads the outputs of every cluster (independent of the layout parameters).
    std::vector<std::array<std::uint32_t, 3>> pr_ref(nc), rx_ref(nc); // (node index j, argument) packed: j * 8 + a
    for (std::uint32_t c = 0; c < nc; ++c) {
        for (std::uint32_t i = 0; i < 3u; ++i) {
            for (int kind = 0; kind < 2; ++kind) {
                const auto u = pl.clusters[c][kind == 0 ? pp.pr[i] : static_cast<std::uint32_t>(pp.rx[i])];
                std::uint32_t ref = ~0u;
                for (std::size_t j = 0; j < grp.nodes.size(); ++j) {
                    const auto &nd = p.nodes[grp.nodes[j] - n_eq];
                    for (std::uint32_t a = 0; a < n_args; ++a) {
                        if (nd.args[a].idx == u) {
                            ref = static_cast<std::uint32_t>(j) * 8u + a;
                        }
                    }
                }
                (kind == 0 ? pr_ref : rx_ref)[c][i] = ref;
            }
        }
    }
    // (The three stores of a lane must differ by the block distance: same rank and argument for the three coordinates.)
    for (std::uint32_t c = 0; c < nc && wide_rd; ++c) {
        for (const auto *ref : {&pr_ref, &rx_ref}) {
            const auto r0 = (*ref)[c][0];
            for (std::uint32_t i = 0; i < 3u; ++i) {
                const auto ri = (*ref)[c][i];
                if (ri == ~0u || r0 == ~0u) {
                    wide_rd = wide_rd && ri == r0; // (unread outputs: all three or none)
                    continue;
                }
                wide_rd = wide_rd && node_coord[ri / 8u] == i && node_rank[ri / 8u] == node_rank[r0 / 8u] && ri % 8u == r0 % 8u;
            }
        }
    }
    const auto ref_slot = [&](std::uint32_t ref) { return op_slot(node_coord[ref / 8u], node_rank[ref / 8u], ref % 8u); };
    const auto addr_lists = [&]() {
        std::vector<lds_op> ops;
        // Position reads of the pair lanes: per side a ds_read_b128 (x, y) and a ds_read_b64 (z).
        for (std::uint32_t sd = 0; sd < (vexch ? 0u : 2u); ++sd) {
            lds_op o16{16, std::vector<std::uint32_t>(pl.L)}, o8{8, std::vector<std::uint32_t>(pl.L)};
            for (std::uint32_t l = 0; l < pl.L; ++l) {
                const auto c = l < nc ? l : 0u;
                const auto tr = body_vars(c, sd);
                const auto b = static_cast<std::uint32_t>(std::find(bodies.begin(), bodies.end(), tr) - bodies.begin());
                o16.addr[l] = pos_base + 4u * b;
                o8.addr[l] = pos_base + 4u * b + 2u;
            }
            ops.push_back(std::move(o16));
            ops.push_back(std::move(o8));
        }
        // Operand reads of the glue rounds.
        const auto n_nodes = static_cast<std::uint32_t>(grp.nodes.size());
        for (std::uint32_t r = 0; r * pl.L < n_nodes; ++r) {
            for (std::uint32_t a = 0; a < n_args; a += 2u) {
                lds_op o{a + 1u < n_args ? 16 : 8, std::vector<std::uint32_t>(pl.L)};
                for (std::uint32_t l = 0; l < pl.L; ++l) {
                    const auto j = r * pl.L + l < n_nodes ? r * pl.L + l : r * pl.L;
                    o.addr[l] = op_slot(node_coord[j], node_rank[j], a);
                }
                ops.push_back(std::move(o));
            }
            // The position coefficients which the round publishes.
            if (vexch) {
                continue;
            }
            lds_op ow{-8, std::vector<std::uint32_t>(pl.L)};
            for (std::uint32_t l = 0; l < pl.L; ++l) {
                if (r * pl.L + l >= n_nodes) {
                    ow.addr[l] = pos_sz + 2u * Dd + blk_used; // (the dummy area)
                    continue;
                }
                const auto j = r * pl.L + l;
                // (The position variable attached to the node: second member of its chain.)
                const auto &ch = att.at(grp.nodes[j]);
                std::uint32_t slot = 0;
                for (const auto var : ch) {
                    for (std::uint32_t b = 0; b < nb; ++b) {
                        for (std::uint32_t i = 0; i < 3u; ++i) {
                            if (bodies[b][i] == var) {
                                slot = pos_base + 4u * b + i;
                            }
                        }
                    }
                }
                ow.addr[l] = slot;
            }
            ops.push_back(std::move(ow));
        }
        // Stores of the products and of the reactions.
        for (int kind = 0; kind < 2; ++kind) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                lds_op o{-8, std::vector<std::uint32_t>(pl.L)};
                for (std::uint32_t l = 0; l < pl.L; ++l) {
                    const auto ref = l < nc ? (kind == 0 ? pr_ref : rx_ref)[l][i] : ~0u;
                    o.addr[l] = ref != ~0u ? ref_slot(ref) : (kind == 0 ? dummy_pr(i) : dummy_rx(i));
                }
                ops.push_back(std::move(o));
            }
        }
        return ops;
    };
    // Bank model (MI355X_MICROARCH.md, LDS): lane groups per instruction width, banks of 4 bytes; identical addresses
    // broadcast, every further distinct address on a busy bank costs the group one more LDS cycle.
    static const std::vector<std::vector<std::uint32_t>> grp128 = [] {
        std::vector<std::vector<std::uint32_t>> g(4);
        const std::uint32_t r0[] = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27};
        const std::uint32_t r1[] = {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31};
        for (const auto x : r0) {
            g[0].push_back(x);
            g[2].push_back(x + 32u);
        }
        for (const auto x : r1) {
            g[1].push_back(x);
            g[3].push_back(x + 32u);
        }
        return g;
    }();
    const auto wcost = [&](const std::vector<lds_op> &ops, std::uint32_t stride) {
        std::uint64_t tot = 0;
        const auto spw_ = 64u / pl.L;
        const auto lane_addr = [&](const lds_op &o, std::uint32_t lane) {
            return ((lane / pl.L) % spw_) * stride + o.addr[lane % pl.L];
        };
        for (const auto &o : ops) {
            const auto n_banks = o.width < 0 ? 32u : 64u;
            const auto dwords = o.width == 16 ? 4u : 2u;
            std::vector<std::vector<std::uint32_t>> groups;
            if (o.width == 16) {
                groups = grp128;
            } else if (o.width == 8) {
                groups.assign(2, {});
                for (std::uint32_t l = 0; l < 64u; ++l) {
                    groups[l / 32u].push_back(l);
                }
            } else {
                groups.assign(4, {});
                for (std::uint32_t l = 0; l < 64u; ++l) {
                    groups[l / 16u].push_back(l);
                }
            }
            for (const auto &g : groups) {
                std::map<std::uint32_t, std::set<std::uint32_t>> banks;
                for (const auto lane : g) {
                    const auto a = lane_addr(o, lane);
                    for (std::uint32_t d = 0; d < dwords; ++d) {
                        banks[(2u * a + d) % n_banks].insert(a);
                    }
                }
                std::size_t mx = 1;
                for (const auto &[b, st_] : banks) {
                    (void)b;
                    mx = std::max(mx, st_.size());
                }
                tot += (mx - 1u) * (o.width < 0 ? 2u : 1u);
            }
        }
        return tot;
    };
    if (wide_rd) {
        // Placement of the operand arrays inside a coordinate block. A ds_write_b64 is serviced in four groups of 16
        // lanes - one system each - over 16 pairs of banks: the 15 pair lanes + 1 idle lane of a system write 16
        // slots, and the store is conflict free iff those slots are distinct modulo 16. With arrays [t0 .. t4, -] back
        // to back no order of the bodies achieves that for the products AND the reactions (the operand positions a
        // sum reads as reactions are the first ones, as products the last ones), and 34 % of the LDS cycles of the
        // kernel were bank conflicts (profiles/r05_outer_ss_sq_counters.json, first collection). The arrays keep
        // the two 16-byte pairs (t0, t1), (t2, t3) adjacent - read with two ds_read_b128 from ONE table register - and
        // let the fifth operand sit anywhere (a second table register): a depth-first search over (array base, place
        // of the fifth operand) per rank finds a placement in which the slots of every product store and of every
        // reaction store are distinct modulo 16 (outer Solar System: a block of 34 slots).
        const auto BLK = 8u * n_rank;
        bool placed = false;
        if (!v5_flag("nostoreplace") && n_args >= 2u && n_args <= 5u) {
            // Which operand positions of a rank are written by the product store / the reaction store.
            std::vector<std::vector<char>> is_rx(n_rank, std::vector<char>(n_args, 0));
            std::vector<std::vector<char>> is_wr(n_rank, std::vector<char>(n_args, 0));
            for (std::uint32_t c = 0; c < nc; ++c) {
                for (int kind = 0; kind < 2; ++kind) {
                    const auto ref = (kind == 0 ? pr_ref : rx_ref)[c][0];
                    if (ref != ~0u) {
                        is_rx[node_rank[ref / 8u]][ref % 8u] = static_cast<char>(kind);
                        is_wr[node_rank[ref / 8u]][ref % 8u] = 1;
                    }
                }
            }
            std::vector<std::vector<std::uint32_t>> cur(n_rank, std::vector<std::uint32_t>(n_args));
            std::vector<char> used(BLK, 0);
            std::uint64_t n_visit = 0;
            const std::function<bool(std::uint32_t, std::uint32_t, std::uint32_t)> dfs = [&](std::uint32_t r, std::uint32_t pm,
                                                                                         std::uint32_t rm) -> bool {
                if (r == n_rank) {
                    // The stores of the idle lanes: a free slot on the one residue each store leaves free.
                    std::uint32_t dz[2] = {~0u, ~0u};
                    for (std::uint32_t z = 0; z < BLK; ++z) {
                        if (used[z] != 0) {
                            continue;
                        }
                        if (dz[0] == ~0u && (pm & (1u << (z % 16u))) == 0u) {
                            dz[0] = z;
                        } else if (dz[1] == ~0u && (rm & (1u << (z % 16u))) == 0u) {
                            dz[1] = z;
                        }
                    }
                    if (dz[0] == ~0u || dz[1] == ~0u) {
                        return false;
                    }
                    dummy_pos[0] = dz[0];
                    dummy_pos[1] = dz[1];
                    return true;
                }
                const auto n_pair = n_args & ~1u; // operands read in 16-byte pairs
                for (std::uint32_t e_ = 0; e_ + n_pair <= BLK; e_ += 2u) {
                    for (std::uint32_t f_ = 0; f_ < (n_args % 2u == 1u ? BLK : 1u); ++f_) {
                        if (++n_visit > 4000000u) {
                            return false;
                        }
                        std::vector<std::uint32_t> ps(n_args);
                        bool ok = true;
                        for (std::uint32_t a_ = 0; a_ < n_args; ++a_) {
                            ps[a_] = a_ < n_pair ? e_ + a_ : f_;
                            ok = ok && used[ps[a_]] == 0 && !(a_ >= n_pair && f_ >= e_ && f_ < e_ + n_pair);
                        }
                        if (!ok) {
                            continue;
                        }
                        std::uint32_t pm2 = pm, rm2 = rm;
                        for (std::uint32_t a_ = 0; a_ < n_args && ok; ++a_) {
                            if (is_wr[r][a_] == 0) {
                                continue;
                            }
                            auto &m_ = is_rx[r][a_] != 0 ? rm2 : pm2;
                            const auto bit = 1u << (ps[a_] % 16u);
                            ok = (m_ & bit) == 0u;
                            m_ |= bit;
                        }
                        if (!ok) {
                            continue;
                        }
                        for (const auto x : ps) {
                            used[x] = 1;
                        }
                        cur[r] = ps;
                        if (dfs(r + 1u, pm2, rm2)) {
                            return true;
                        }
                        for (const auto x : ps) {
                            used[x] = 0;
                        }
                    }
                }
                return false;
            };
            if (pl.L == 16u && dfs(0, 0, 0)) {
                arr_pos = cur;
                placed = true;
            }
        }
        if (placed) {
            blk_used = std::max(dummy_pos[0], dummy_pos[1]) + 1u;
            for (const auto &v : arr_pos) {
                for (const auto x : v) {
                    blk_used = std::max(blk_used, x + 1u);
                }
            }
            blk_used = (blk_used + 1u) & ~1u;
        }
        std::uint64_t best_c = ~std::uint64_t(0);
        std::uint32_t best_D = Dd, best_stride = 0;
        // (+ 2: the dummy area behind the arrays - idle lanes of a partially filled glue round publish there.)
        const auto total_for = [&](std::uint32_t D_) { return pos_sz + 2u * D_ + blk_used + 2u + (bk_in_slab ? 16u : 0u); };
        // The distance between the coordinate blocks and between the slabs of two systems: scanned with the bank model
        // (reads in the lane groups of each instruction width; the stores are settled by the placement above).
        for (std::uint32_t D_ = blk_used; D_ <= blk_used + 6u; D_ += 2u) {
            Dd = D_;
            const auto ops = addr_lists();
            const auto tot = total_for(D_);
            for (std::uint32_t st_ = (tot + 1u) & ~1u; st_ < ((tot + 1u) & ~1u) + 32u; st_ += 2u) {
                const auto c = wcost(ops, st_);
                if (c < best_c) {
                    best_c = c;
                    best_D = D_;
                    best_stride = st_;
                }
            }
        }
        Dd = best_D;
        slab_stride_opt = best_stride;
        bank_cost = best_c;
        if (v5_flag("bankdbg")) {
            const auto ops = addr_lists();
            std::fprintf(stderr, "wide layout: D = %u, stride = %u, cost = %llu, perm =", Dd, best_stride,
                         static_cast<unsigned long long>(best_c));
            for (std::uint32_t x = 0; x < n_rank; ++x) {
                std::fprintf(stderr, " %u", x);
            }
            std::fprintf(stderr, "\n");
            for (const auto &o : ops) {
                std::fprintf(stderr, "  width %d cost %llu addr:", o.width,
                             static_cast<unsigned long long>(wcost(std::vector<lds_op>{o}, best_stride)));
                for (const auto x : o.addr) {
                    std::fprintf(stderr, " %u", x);
                }
                std::fprintf(stderr, "\n");
            }
        }
        // The slots.
        std::fill(pl.slot_of.begin(), pl.slot_of.end(), -1);
        for (std::uint32_t b = 0; b < nb && !vexch; ++b) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                pl.slot_of[bodies[b][i]] = static_cast<int>(pos_base + 4u * b + i);
            }
        }
        wide_pr.assign(pl.L, {});
        wide_rx.assign(pl.L, {});
        for (std::uint32_t l = 0; l < pl.L; ++l) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                const auto rp = l < nc ? pr_ref[l][i] : ~0u, rr = l < nc ? rx_ref[l][i] : ~0u;
                wide_pr[l][i] = rp != ~0u ? ref_slot(rp) : dummy_pr(i);
                wide_rx[l][i] = rr != ~0u ? ref_slot(rr) : dummy_rx(i);
                if (l < nc && rp != ~0u) {
                    pl.slot_of[pl.clusters[l][pp.pr[i]]] = static_cast<int>(wide_pr[l][i]);
                }
                if (l < nc && rr != ~0u) {
                    pl.slot_of[pl.clusters[l][static_cast<std::uint32_t>(pp.rx[i])]] = static_cast<int>(wide_rx[l][i]);
                }
            }
        }
        pl.n_slots = total_for(Dd) - 2u - (bk_in_slab ? 16u : 0u);
    }
}

// Lane-reduced sums (stage 0c, after frx has put the plain sums last). With the reactions fused, a first-round sum reads
// the raw direct product of a pair and scales it itself - so the terms of a plain sum of the later rounds sit, unscaled,
// in a register of the first-round lanes which read them, and the sum can be formed by additions across those lanes
// instead of LDS reads (5 reads, a fifth of the reads of an order for the outer Solar System). Applies when every later
// sum has 5 terms, each term is read by exactly one first-round sum at ONE common operand position, and the first-round
// sums can be put on the lanes so that the holders of every later sum are 5 adjacent lanes of one 16-lane row in its
// argument order: three row_shr steps on that one register (emit_glue_compute()) then reproduce the pairwise tree
// ((t0 + t1) + (t2 + t3)) + t4 on the last lane of each segment - all the later sums at once. Anything else declines
// (no per-lane operand select, no other term count). Leaves lane_sum, ls_first, ls_last, ls_pos.
void cluster2_gen::plan_lane_sums(std::uint32_t n_first)
{
    constexpr std::uint32_t n_terms = 5;
    const auto &nodes = pl.groups[0].nodes;
    const auto n_nodes = static_cast<std::uint32_t>(nodes.size());
    if (n_nodes <= L || n_first >= n_nodes || n_first > L) {
        return;
    }
    // (What a sum reads in the place of a cluster output: the direct product.)
    std::map<std::uint32_t, std::uint32_t> raw_of;
    for (std::uint32_t c = 0; c < nc; ++c) {
        for (std::uint32_t i = 0; i < 3u; ++i) {
            raw_of[pl.clusters[c][pp.pr[i]]] = pl.clusters[c][pp.pr[i]];
            raw_of[pl.clusters[c][static_cast<std::uint32_t>(pp.rx[i])]] = pl.clusters[c][pp.pr[i]];
        }
    }
    std::map<std::uint32_t, std::pair<std::uint32_t, std::uint32_t>> holder; // product -> (first-round node, operand position)
    std::set<std::uint32_t> shared;
    for (std::uint32_t j = 0; j < n_first; ++j) {
        const auto &args = p.nodes[nodes[j] - n_eq].args;
        for (std::uint32_t a = 0; a < args.size(); ++a) {
            const auto u = raw_of.at(args[a].idx);
            if (!holder.emplace(u, std::make_pair(j, a)).second) {
                shared.insert(u);
            }
        }
    }
    std::vector<std::uint32_t> first_lanes, last_lanes;
    std::vector<char> taken(n_first, 0);
    std::uint32_t pos = ~0u;
    for (std::uint32_t j = n_first; j < n_nodes; ++j) {
        const auto &args = p.nodes[nodes[j] - n_eq].args;
        const auto l0 = static_cast<std::uint32_t>(first_lanes.size());
        if (args.size() != n_terms || l0 % 16u + n_terms > std::min(L, 16u)) {
            return;
        }
        for (const auto &o : args) {
            const auto it = holder.find(o.idx);
            if (it == holder.end() || shared.count(o.idx) != 0u || taken[it->second.first] != 0
                || (pos != ~0u && it->second.second != pos)) {
                return;
            }
            pos = it->second.second;
            taken[it->second.first] = 1;
            first_lanes.push_back(it->second.first);
        }
        last_lanes.push_back(l0 + n_terms - 1u);
    }
    for (std::uint32_t j = 0; j < n_first; ++j) {
        if (taken[j] == 0) {
            first_lanes.push_back(j);
        }
    }
    ls_first.assign(L, ~0u);
    ls_last.assign(L, ~0u);
    std::copy(first_lanes.begin(), first_lanes.end(), ls_first.begin());
    for (std::size_t s = 0; s < last_lanes.size(); ++s) {
        ls_last[last_lanes[s]] = n_first + static_cast<std::uint32_t>(s);
    }
    ls_pos = pos;
    // Where a lane without a later sum parks the store of that round: a column of the first round - the store of the first
    // round, issued behind it, overwrites every one of them. Its own, unless the bank pair of that column (column mod 16: a
    // ds_write_b64 is serviced per 16 lanes, the lanes of a system share the offset of its row) is the one of a later sum's
    // column or already taken: then a free one.
    ls_park.assign(L, ~0u);
    std::set<std::uint32_t> banks;
    for (const auto j : ls_last) {
        if (j != ~0u) {
            banks.insert(j % 16u);
        }
    }
    for (std::uint32_t l = 0; l < L; ++l) {
        if (ls_last[l] == ~0u && ls_first[l] != ~0u && banks.insert(ls_first[l] % 16u).second) {
            ls_park[l] = ls_first[l];
        }
    }
    for (std::uint32_t l = 0; l < L; ++l) {
        for (std::uint32_t j = 0; ls_last[l] == ~0u && ls_park[l] == ~0u && j < n_first; ++j) {
            if (banks.insert(j % 16u).second) {
                ls_park[l] = j;
            }
        }
        if (ls_last[l] == ~0u && ls_park[l] == ~0u) {
            ls_park[l] = ls_first[l] != ~0u ? ls_first[l] : ls_first[0];
        }
    }
    // The invariant the parked stores rest on: every parked column is the column of a lane which owns a first-round node,
    // i.e. one which the store of the first round - emitted behind the reduced round's, emit_step_body() - writes at every order.
    for (std::uint32_t l = 0; l < L; ++l) {
        if (ls_last[l] == ~0u && std::find(first_lanes.begin(), first_lanes.end(), ls_park[l]) == first_lanes.end()) {
            throw std::logic_error("hy_taylor (one lane per pair): a store of the lane-reduced round is parked on a column which "
                                   "the first round does not overwrite");
        }
    }
    lane_sum = true;
}

std::uint32_t cluster2_gen::n_rounds_of(std::size_t g) const
{
    return (lane_sum && g == 0u) ? 2u : (static_cast<std::uint32_t>(pl.groups[g].nodes.size()) + L - 1u) / L;
}

std::pair<std::uint32_t, bool> cluster2_gen::round_node(std::size_t g, std::uint32_t r, std::uint32_t l) const
{
    if (lane_sum && g == 0u) {
        // (A lane without a later sum replicates a first-round node there - ls_park -, the idle lanes of the first round lane 0.)
        if (r == 1u) {
            return ls_last[l] != ~0u ? std::make_pair(ls_last[l], true) : std::make_pair(ls_park[l], false);
        }
        return ls_first[l] != ~0u ? std::make_pair(ls_first[l], true) : std::make_pair(ls_first[0], false);
    }
    const auto n_nodes = static_cast<std::uint32_t>(pl.groups[g].nodes.size());
    const auto j = r * L + l;
    return j < n_nodes ? std::make_pair(j, true) : std::make_pair(r * L, false);
}

// ---- 3. Tables. ----
std::size_t cluster2_gen::add_utbl(std::vector<std::uint32_t> v, bool is_slot)
{
    // Deduplicate identical tables.
    for (std::size_t t = 0; t < utbl.size(); ++t) {
        if (utbl[t] == v && (utbl_is_slot[t] != 0) == is_slot) {
            return t;
        }
    }
    std::string ex = "ut" + std::to_string(utbl.size());
    for (std::size_t t = 0; one_lane && is_slot && t < utbl.size(); ++t) {
        if (utbl_is_slot[t] == 0 || utexpr[t] != "ut" + std::to_string(t)) {
            continue;
        }
        const auto d = static_cast<std::int64_t>(v[0]) - static_cast<std::int64_t>(utbl[t][0]);
        bool affine = true;
        for (std::size_t l2 = 0; l2 < v.size(); ++l2) {
            affine = affine && (static_cast<std::int64_t>(v[l2]) - static_cast<std::int64_t>(utbl[t][l2]) == d);
        }
        if (affine) {
            ex = "(ut" + std::to_string(t) + (d >= 0 ? " + " : " - ") + std::to_string(d >= 0 ? d : -d) + "u)";
            break;
        }
    }
    utexpr.push_back(std::move(ex));
    utbl.push_back(std::move(v));
    utbl_is_slot.push_back(is_slot ? 1 : 0);
    return utbl.size() - 1u;
}

std::size_t cluster2_gen::add_dtbl(std::vector<double> v)
{
    dtbl.push_back(std::move(v));
    return dtbl.size() - 1u;
}

// Slab slot through which a product pr travels (its own, or - when only its reaction was exported - that one's).
std::uint32_t cluster2_gen::pr_slot(std::uint32_t pr_u, std::uint32_t rx_u, std::uint32_t dflt) const
{
    if (pl.slot_of[pr_u] >= 0) {
        return static_cast<std::uint32_t>(pl.slot_of[pr_u]);
    }
    return (fuse_rx && pl.slot_of[rx_u] >= 0) ? static_cast<std::uint32_t>(pl.slot_of[rx_u]) : dflt;
}

std::string cluster2_gen::lane_par(std::vector<std::uint32_t> idx)
{
    const auto t = add_utbl(std::move(idx), false);
    if (std::find(lane_par_tbls.begin(), lane_par_tbls.end(), t) == lane_par_tbls.end()) {
        lane_par_tbls.push_back(t);
    }
    return "lp" + std::to_string(t);
}

// Final evaluation of a partially filled owner slot with a derived variable (x' = v; 18 velocity columns on 16 lanes
// leave 2): ONE series per lane - the lanes [0, n) sum the velocity columns, the lanes [n, 2 n) the series derived from
// them, whose coefficient k is row k - 1 of the same column times RN(1 / k). Both kinds run the same statements: where
// the lane's current value lives, where row k of its series starts and which row of the factor table (ones / RN(1 / k))
// it reads are per-lane table entries (pk_tbl[owner slot] = the three tables).
bool cluster2_gen::pack_tail_slot(const owner_slot &ow, const owner_slot *dv) const
{
    return one_lane && jet_lds && !m4 && opts.high_accuracy && dv != nullptr && !ow.derived && 2u * ow.n_valid <= L
           && !v5_flag("nopack2");
}

} // namespace heyoka_amd::cluster2_detail
