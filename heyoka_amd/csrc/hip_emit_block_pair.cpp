// Block mode, the pair phase ("v2 cluster phase"): the whole step body for decompositions whose clusters are point-mass
// pairs (pair_phase_applicable(), hip_emit_block.cpp). The stages of block_gen (hip_emit_block_gen.hpp) which produce it.
//
// Index pairs ("slots"): at order k the convolutions of the cluster run over the pairs (i, p = k - i), 0 <= i <= p. Slot 0
// pairs the order-0 coefficients with the order-k ones (which are being computed), slots 1 .. floor(k / 2) pair known
// coefficients; for an even k the last slot is the middle term (i = p), entered with the weights (1/2, 0) on the symmetric
// parts.
//   r2^[k]  = 2 * sum_i d^[i] . d^[p]                                                   (src/detail/sum_sq.cpp:100-245)
//   pw^[k]  = (sum_j (k a - j (a + 1)) r2^[k-j] pw^[j]) / (k r2^[0])                   (src/math/pow.cpp:395-550)
//   f_c^[k] = sum_j d_c^[k-j] pw^[j]                                                    (src/math/prod.cpp:314-395)
// Data of a slot: r2^[i], pw^[i] from the registers (i < M) or the tape, r2^[p], pw^[p] from the tape, d^[i], d^[p]
// recomputed from the jets of the external inputs in LDS (rows stored in REVERSE order, so that the row of p = k - i
// is a non-negative constant offset from the row of k). All the tape loads of a round are issued, unconditionally
// (rows of slots beyond the last one are clamped to a row which is loaded anyway), one round ahead of their use.
//
// The switches named in the comments below are those of HEYOKA_AMD_BLOCK_OPTS: the list is in hip_emit_block_gen.hpp.
#include <algorithm>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "hip_emit_block_gen.hpp"

namespace heyoka_amd::block_detail
{

using namespace cluster_detail;

// ---- stage 6a: the parameters of the phase; false: not a pair phase after all (nothing has been written) ----
bool block_gen::pair_parameters()
{
    R = n_iter;
    P = order;
    // Developer experiments (timing only, wrong results): switch exp.
    exp_mode = sw.exp;
    M = 160u / (4u * R);
    // Two wavefronts per SIMD: 96 registers for rows which stay in registers - the low rows 0 ... M - 1 for the whole step
    // and the `hand` most recent ones, handed over from order to order (below). A low row m saves 20 - 2 m tape reads per
    // step, a handed-over row h 21 - 2 h: dealt in turn (row 0, m = 1, h = 2, m = 2, h = 3, ...).
    std::uint32_t hand_dflt = 1;
    // (More than four rounds per lane - nbody(80): seven -: per-round registers cost too much, measured: spills inside
    // the order loop halve the rate; two rows, one hand-over, no differences / descriptors kept.)
    lean = two_waves && R > 4u;
    if (lean) {
        M = std::max(2u, 80u / (4u * R));
    } else if (two_waves) {
        const auto rows = std::max(3u, 96u / (4u * R));
        M = 1;
        for (std::uint32_t i = 0; i + 1u < rows; ++i) {
            if (i % 2u == 0u) {
                ++M;
            } else {
                ++hand_dflt;
            }
        }
    }
    M = static_cast<std::uint32_t>(sw.M.value_or(static_cast<int>(M)));
    M = std::min(T, std::max(2u, M));
    // The high member p = k - i of slot i is one of the rows in registers while k < i + M (slots 2 ... M - 1 of the orders
    // 2 i ... i + M - 1): selected from the register copies by the (wave-uniform) order, not loaded. The rows < M are
    // then never read from the tape and not stored; neither is the row of order P - 2, which only order P - 1 reads -
    // from the hand-over registers. 11 of the 120 row transfers of a step of nbody(64) (rows < 5 in registers).
    reg_high = sw.reg_high != 0 && exp_mode == 0;
    // (reg_high=2: the selection behind a wave-uniform branch at the head of the slot - no instruction at the orders
    // whose high member comes from the tape.)
    reg_high_br = sw.reg_high == 2;
    // Quotients as products with reciprocals + one exact-residual correction unless kw::exact_division (switch div: A/B).
    recip = !opts.exact_division && sw.div == 0;
    int s_sq = -1, s_pw = -1;
    for (std::uint32_t s = 0; s < n_sto; ++s) {
        if (recomp[s] == 0 && pl.stored_pos[s] == pp.sq) {
            s_sq = static_cast<int>(s);
        }
        if (recomp[s] == 0 && pl.stored_pos[s] == pp.pw) {
            s_pw = static_cast<int>(s);
        }
    }
    for (std::uint32_t c = 0; c < 3u; ++c) {
        for (std::uint32_t x = 0; x < n_out; ++x) {
            if (pl.out_pos[x] == pp.pr[c]) {
                io_of[c] = static_cast<int>(x);
            }
        }
        for (std::uint32_t s = 0; s < n_sto; ++s) {
            if (pl.stored_pos[s] == pp.d[c] && recomp[s] == 0) {
                return false;
            }
        }
    }
    if (s_sq < 0 || s_pw < 0 || io_of[0] < 0 || io_of[1] < 0 || io_of[2] < 0 || n_ext > 8u) {
        return false;
    }
    arow0 = static_cast<std::uint64_t>(tape_row[static_cast<std::uint32_t>(s_sq)]) * order;
    brow0 = static_cast<std::uint64_t>(tape_row[static_cast<std::uint32_t>(s_pw)]) * order;
    // (Switch split: A/B harness - the two tape members in separate halves of the tape, two 8-byte accesses.)
    il_tape = sw.split == 0 && sw.xpf == 0 && n_tape == 2u;
    rowb = static_cast<std::uint64_t>(ncp) * 8u;
    ejrow = static_cast<std::uint64_t>(n_ej) * 8u;     // bytes per row of the input jets
    ej0b = static_cast<std::uint64_t>(P - 1u) * ejrow; // row of order 0
    ex = pp.ex;
    e1 = pp.ex + 1.;
    // (Switch unpacked: A/B harness - one table per operand position, eight 2-byte reads per node.)
    packed_idx = !wide && sw.unpacked == 0;
    pair_resolve_pipeline(hand_dflt);
    return true;
}

// The software pipeline of the orders 1 .. P - 1 (pair_order_loop()): the switches whose defaults depend on the geometry.
void block_gen::pair_resolve_pipeline(std::uint32_t hand_dflt)
{
    // Rounds per pipeline group (the accumulators, descriptors and tape registers of a group are live at the same
    // time: R rounds at once do not fit the register file next to the register copies of the low orders).
    G = R;
    if (R > 4u) {
        G = 4;
    }
    if (two_waves) {
        G = 2;
    }
    G = static_cast<std::uint32_t>(sw.G.value_or(static_cast<int>(G)));
    G = std::max(1u, std::min(G, R));
    // Depth of the tape-load pipeline, in slots: the loads of slot i + D are issued at the head of slot i. One slot of a
    // group is G * ~80 instructions, i.e. a fraction of a microsecond, against 1 - 2 us for a load which misses L2.
    // (Measured on nbody(64), 65 536 systems, rows < 5 in registers: depth 1 / 2 / 3 / 4 with groups of two rounds =
    // 9.8e5 / 9.7e5 / 8.8e5 / 8.6e5 system-steps/s - the registers of a deeper pipeline cost more than the latency they
    // hide; the kernel is bound by the instruction issue of its single wavefront per SIMD.)
    D = static_cast<std::uint32_t>(std::max(1, sw.D.value_or(two_waves ? 2 : 1)));
    // Cross-group prefetch (switch xpf): the high rows of the slots 2 .. D + 1 of a group - rows of order <= k - 2, stored long
    // ago - are requested while the PREVIOUS group finishes (for the first group of an order: behind the last group of
    // the order before, across the glue phases), so that a group does not start with the latency of the memory system
    // exposed (D slots of two rounds are ~0.5 us of work against 1 - 2 us): registers xa<i>_<q> / xb<i>_<q>, q the
    // position of the round in its group, live from the end of a group to the slots of the next one.
    xpf = sw.xpf != 0 && D + 1u < M && D + 1u < T && !reg_high && exp_mode == 0 && R % G == 0u;
    // (Switch hand=H: the coefficients of the orders k - 2 ... k - H handed over in registers too: the slots 2 ... H need no
    // tape load for their high member.)
    hand = (!xpf && !reg_high && exp_mode == 0)
               ? std::min<std::uint32_t>(static_cast<std::uint32_t>(std::max(1, sw.hand.value_or(static_cast<int>(hand_dflt)))), std::min(T - 1u, il_tape ? T - 1u : M - 1u))
               : 1u;
    // (Switch hoist, A/B harness: the descriptors of the clusters of a lane loaded once per step, in registers through the orders.)
    hoist = sw.hoist.value_or(two_waves && !lean ? 1 : 0) != 0;
    // (Switch keepdz: the order-0 differences of the clusters of a lane in registers through the orders - they are read
    // twice per order and round otherwise.)
    keepdz = sw.keepdz.value_or(two_waves && !lean ? 1 : 0) != 0;
    // (Switch nopp, A/B harness: no ping-pong - the LDS reads of a step right in front of its arithmetic, one register set.)
    nopp = sw.nopp.value_or(two_waves ? 1 : 0) != 0;
}

// ---- stage 6b: the descriptors of the clusters and the declarations which live as long as the kernel ----
void block_gen::pair_descriptors()
{
    {
        // State variable -> index of its jet among the LDS-resident input jets (0xffff: not an input of the clusters).
        std::vector<std::uint32_t> sv_ej(n_eq, 0xffffu);
        for (std::uint32_t e2 = 0; e2 < n_ej; ++e2) {
            sv_ej[ej_slots[e2]] = e2;
        }
        emit_utbl("hy_sv_ej", sv_ej);
    }
    // ---- the descriptors of the clusters: byte offsets (inside a row of the input jets) of the external inputs, two
    // per word, and the slab slots of the outputs; loaded at the head of the tape loads of a round (a table of
    // (n_dq + 2) * n_clusters words shared by all the workgroups: L2) - as values which live for the whole kernel they
    // were spilled, and a scratch reload inside the order loop makes the wavefront wait for ALL its outstanding tape
    // loads (loads, stores and scratch accesses share one in-order counter).
    decl << "#define HY_EJ(off) (*(const double *)((const char *)ejet + (off)))\n";
    decl << "#define HY_EJW(off) (*(double *)((char *)ejet + (off)))\n";
    // Tape accesses as raw buffer instructions: lane offset in a VGPR, row offset in an SGPR - one instruction per access
    // (the flat form costs a 64-bit VALU addition per access and two SALU instructions per row).
    decl << "typedef unsigned hy_u2 __attribute__((ext_vector_type(2)));\n";
    decl << "typedef unsigned hy_u4 __attribute__((ext_vector_type(4)));\n";
    decl << "const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc((void *)tape, 0, "
         << static_cast<std::uint64_t>(n_tape) * order * ncp * 8u << ", 0x00020000);\n";
    decl << "#define HY_TLD(lo, so) __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(trs, (lo), (so), 0))\n";
    decl << "#define HY_TST(v, lo, so) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(hy_u2, (v)), trs, (lo), (so), 0)\n";
    // Interleaved tape (round 6): the coefficients of the two tape members of a cluster side by side,
    // tape[(row * n_clusters + cluster) * 2 + member] - ONE 16-byte load / store per cluster and row instead of two 8-byte ones.
    decl << "typedef double hy_dd2 __attribute__((ext_vector_type(2)));\n";
    decl << "#define HY_TLD2(lo, so) __builtin_bit_cast(hy_dd2, __builtin_amdgcn_raw_buffer_load_b128(trs, (lo), (so), 0))\n";
    decl << "#define HY_TST2(va, vb, lo, so) { hy_dd2 t2_; t2_[0] = (va); t2_[1] = (vb); __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(hy_u4, t2_), trs, (lo), (so), 0); }\n";
    // Compact form (2 words per cluster instead of n_ext / 2 + 2) when the tables are affine: the inputs of a cluster are
    // the coordinates of two bodies whose jets sit at a constant distance from one another ([component][body] layout of
    // the input jets) and its outputs sit at constant distances too - then one offset per body and one output slot
    // describe the cluster, the rest are constants which fold into the offset fields of the LDS instructions (and the
    // three components of a body share ONE address addition per row instead of three).
    ex_word.assign(n_ext, 0u);
    ex_shift.assign(n_ext, 0u);
    ex_delta.assign(n_ext, 0u);
    compact = n_ext == 6u;
    if (compact) {
        for (std::uint32_t side = 0; side < 2u && compact; ++side) {
            const auto xb = pp.de[0][side];
            for (std::uint32_t comp = 0; comp < 3u && compact; ++comp) {
                const auto x = pp.de[comp][side];
                const auto d0 = static_cast<std::int64_t>(ej_index[static_cast<std::size_t>(x) * nc])
                                - static_cast<std::int64_t>(ej_index[static_cast<std::size_t>(xb) * nc]);
                for (std::uint32_t c = 0; c < nc && compact; ++c) {
                    compact = static_cast<std::int64_t>(ej_index[static_cast<std::size_t>(x) * nc + c])
                                  - static_cast<std::int64_t>(ej_index[static_cast<std::size_t>(xb) * nc + c])
                              == d0;
                }
                compact = compact && d0 >= 0;
                ex_word[x] = 0;
                ex_shift[x] = 16u * side;
                ex_delta[x] = static_cast<std::uint32_t>(d0) * 8u;
            }
        }
        for (std::uint32_t q = 1; q < 3u && compact; ++q) {
            const auto d0 = static_cast<std::int64_t>(oslot_of(0, io_of[q])) - static_cast<std::int64_t>(oslot_of(0, io_of[0]));
            for (std::uint32_t c = 0; c < nc && compact; ++c) {
                compact = static_cast<std::int64_t>(oslot_of(c, io_of[q])) - static_cast<std::int64_t>(oslot_of(c, io_of[0])) == d0;
            }
            compact = compact && d0 >= 0;
            out_delta[q] = static_cast<std::uint32_t>(d0);
        }
    }
    if (!compact) {
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            ex_word[x] = x / 2u;
            ex_shift[x] = 16u * (x % 2u);
            ex_delta[x] = 0;
        }
    }
    n_dq = compact ? 1u : (n_ext + 1u) / 2u; // words holding input offsets
    n_dw = compact ? 2u : n_dq + 2u;          // words per cluster
    {
        std::vector<std::uint32_t> dsc(static_cast<std::size_t>(n_dw) * nc, 0u);
        for (std::uint32_t c = 0; c < nc; ++c) {
            if (compact) {
                dsc[c] = (ej_index[static_cast<std::size_t>(pp.de[0][0]) * nc + c] * 8u)
                         | ((ej_index[static_cast<std::size_t>(pp.de[0][1]) * nc + c] * 8u) << 16);
                dsc[static_cast<std::size_t>(nc) + c] = oslot_of(c, io_of[0]);
            } else {
                for (std::uint32_t x = 0; x < n_ext; ++x) {
                    dsc[static_cast<std::size_t>(x / 2u) * nc + c]
                        |= (ej_index[static_cast<std::size_t>(x) * nc + c] * 8u) << (16u * (x % 2u));
                }
                dsc[static_cast<std::size_t>(n_dq) * nc + c] = oslot_of(c, io_of[0]) | (oslot_of(c, io_of[1]) << 16);
                dsc[static_cast<std::size_t>(n_dq + 1u) * nc + c] = oslot_of(c, io_of[2]);
            }
        }
        tbl << "__device__ const unsigned hy_dsc[" << dsc.size() << "] = {";
        for (const auto x : dsc) {
            tbl << x << ",";
        }
        tbl << "};\n";
    }
    // NOTE: the idle lanes of a partial last round work on a copy of the last cluster and store the same values to the
    // same places as the lane which owns it: no predicated stores, i.e. no divergent control flow in the cluster phase
    // (see the toolchain note on exec-masked regions under register pressure, heyoka_amd/codegen_check.py).
    for (std::uint32_t r = 0; r < R; ++r) {
        const bool full = static_cast<std::uint64_t>(r + 1u) * bs <= nc;
        if (!full) {
            decl << "const bool live_" << r << " = tid + " << r * bs << "u < " << nc << "u;\n";
        }
    }
}

std::string block_gen::ex_expr(std::uint32_t x, std::uint32_t r) const
{
    const auto w = "dq_" + S(ex_word[x]) + "_" + S(r);
    auto ret = ex_shift[x] == 0u ? "(" + w + " & 0xffffu)" : "(" + w + " >> 16)";
    if (ex_delta[x] != 0u) {
        ret = "(" + ret + " + " + U(ex_delta[x]) + ")";
    }
    return ret;
}

std::string block_gen::out_expr(std::uint32_t q, std::uint32_t r) const
{
    if (compact) {
        return "(dq_1_" + S(r) + " + " + U(out_delta[q]) + ")";
    }
    if (q == 0u) {
        return "(dq_" + S(n_dq) + "_" + S(r) + " & 0xffffu)";
    }
    return q == 1u ? "(dq_" + S(n_dq) + "_" + S(r) + " >> 16)" : "dq_" + S(n_dq + 1u) + "_" + S(r);
}

std::string block_gen::cl_expr(std::uint32_t r) const
{
    const bool full = static_cast<std::uint64_t>(r + 1u) * bs <= nc;
    return full ? "tid + " + U(r * bs) : "(live_" + S(r) + " ? tid + " + U(r * bs) + " : " + U(nc - 1u) + ")";
}

// Cluster index of the lane in round r and its byte offset inside a tape row; the descriptor loads.
void block_gen::desc_loads(std::uint32_t r)
{
    const bool full = static_cast<std::uint64_t>(r + 1u) * bs <= nc;
    // (The empty asm statement keeps the loads where they are: as loop invariants they would be hoisted out of the
    // order loop and spilled.)
    os << "unsigned cl_" << r << " = "
       << (full ? "tid + " + U(r * bs) : "live_" + S(r) + " ? tid + " + U(r * bs) + " : " + U(nc - 1u)) << ";\n";
    os << "asm volatile(\"\" : \"+v\"(cl_" << r << "));\n";
    os << "const unsigned lo_" << r << " = cl_" << r << " * 8u;\n";
    for (std::uint32_t j = 0; j < n_dw; ++j) {
        os << "const unsigned dq_" << j << "_" << r << " = hy_dsc[" << U(static_cast<std::uint64_t>(j) * nc) << " + cl_" << r
           << "];\n";
    }
}

void block_gen::unpack_ex(std::uint32_t r)
{
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        os << "const unsigned ex" << x << " = " << ex_expr(x, r) << ";\n";
    }
}

void block_gen::unpack_out(std::uint32_t r)
{
    os << "const unsigned dvo0 = " << out_expr(0, r) << ", dvo1 = " << out_expr(1, r) << ", dvo2 = " << out_expr(2, r)
       << ";\n";
}

// d_c of the row at byte offset `row` (an expression): minuend - subtrahend (src/detail/sub.cpp:60-124).
void block_gen::diff(const std::string &name, std::uint32_t c, const std::string &row)
{
    os << "const double " << name << " = HY_EJ(" << row << " + ex" << pp.de[c][0] << ") - HY_EJ(" << row << " + ex"
       << pp.de[c][1] << ");\n";
}

void block_gen::store_out(const std::string v[3])
{
    os << "slab[dvo0] = " << v[0] << ";\n";
    os << "slab[dvo1] = " << v[1] << ";\n";
    os << "slab[dvo2] = " << v[2] << ";\n";
}

// ---- stage 6c: the index tables of the glue of this phase ----
// Order of the nodes of a merged level = lane assignment: lane l of a round gathers ITS operands from the slab
// with 64-bit reads, 32 lanes at a time, one cycle per distinct address sharing a bank. In the order of the
// decomposition (the three coordinates of a sum on adjacent lanes, 2016 slots = 0 mod 32 apart; partners in
// triangular order) a gather of the widest level of nbody(64) takes 4.9 cycles per 32 lanes; dealing the
// nodes greedily into groups of 32 with at most `tol` addresses per bank and operand position brings that
// to 2.3 (tol = 2). (Switch noglueperm: A/B harness.)
std::vector<std::uint32_t> block_gen::bank_aware_lane_order(const std::vector<std::uint32_t> &nodes, std::uint32_t nargs) const
{
    const auto slots_of = [this, nargs](std::uint32_t u) {
        std::vector<std::uint32_t> v(nargs, n_slots + 1u);
        const auto &args = p.nodes[u - n_eq].args;
        for (std::uint32_t a2 = 0; a2 < nargs && a2 < args.size(); ++a2) {
            v[a2] = static_cast<std::uint32_t>(pl.slot_of[args[a2].idx]);
        }
        return v;
    };
    const auto score = [&slots_of, nargs](const std::vector<std::uint32_t> &ord) {
        std::uint64_t tot = 0;
        for (std::size_t g0 = 0; g0 < ord.size(); g0 += 32u) {
            for (std::uint32_t a2 = 0; a2 < nargs; ++a2) {
                std::map<std::uint32_t, std::set<std::uint32_t>> bank;
                for (std::size_t j = g0; j < std::min(ord.size(), g0 + 32u); ++j) {
                    const auto sl = slots_of(ord[j])[a2];
                    bank[sl % 32u].insert(sl);
                }
                std::size_t mx = 0;
                for (const auto &[b_, st] : bank) {
                    mx = std::max(mx, st.size());
                }
                tot += mx;
            }
        }
        return tot;
    };
    auto best = nodes;
    auto best_score = score(nodes);
    for (std::uint32_t tol = 1; tol <= 3u; ++tol) {
        std::vector<std::uint32_t> rem = nodes, ord;
        while (!rem.empty()) {
            std::vector<std::uint32_t> grp, keep;
            std::vector<std::map<std::uint32_t, std::set<std::uint32_t>>> bank(nargs);
            for (const auto u : rem) {
                bool ok = grp.size() < 32u;
                std::vector<std::uint32_t> sl;
                if (ok) {
                    sl = slots_of(u);
                    for (std::uint32_t a2 = 0; a2 < nargs && ok; ++a2) {
                        const auto bi = bank[a2].find(sl[a2] % 32u);
                        ok = bi == bank[a2].end() || bi->second.count(sl[a2]) != 0u || bi->second.size() < tol;
                    }
                }
                if (ok) {
                    grp.push_back(u);
                    for (std::uint32_t a2 = 0; a2 < nargs; ++a2) {
                        bank[a2][sl[a2] % 32u].insert(sl[a2]);
                    }
                } else {
                    keep.push_back(u);
                }
            }
            std::size_t taken = 0;
            while (grp.size() < 32u && taken < keep.size()) {
                grp.push_back(keep[taken++]);
            }
            keep.erase(keep.begin(), keep.begin() + static_cast<std::ptrdiff_t>(taken));
            ord.insert(ord.end(), grp.begin(), grp.end());
            rem.swap(keep);
        }
        if (const auto sc = score(ord); sc < best_score) {
            best_score = sc;
            best = ord;
        }
    }
    return best;
}

// Sums of one dependency level with different numbers of terms (63 accelerations terms per body arrive as sums of
// 8 + 8 + ... + 7: seven shapes per level for nbody(64), six of them with 48 nodes on 256 lanes) run as ONE group of
// the widest shape, the missing operands read a slot which holds 0.0: the pairwise tree of the padded sum adds
// exact zeros where the short one has nothing (same value), and a level is 7 + 2 + 2 lane rounds instead of 21.
void block_gen::pair_merged_glue()
{
    group_merged.assign(pl.groups.size(), 0);
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &n0 = p.nodes[pl.groups[g].nodes[0] - n_eq];
        bool all_var = n0.kind == func_kind::sum && n0.args.size() <= 8u;
        for (const auto &o : n0.args) {
            all_var = all_var && is_var(o);
        }
        if (all_var) {
            auto &m = merged[pl.groups[g].level];
            m.groups.push_back(g);
            m.nargs = std::max(m.nargs, static_cast<std::uint32_t>(n0.args.size()));
            m.nodes.insert(m.nodes.end(), pl.groups[g].nodes.begin(), pl.groups[g].nodes.end());
        }
    }
    for (auto it = merged.begin(); it != merged.end();) {
        if (it->second.groups.size() < 2u) {
            it = merged.erase(it);
            continue;
        }
        for (const auto g : it->second.groups) {
            group_merged[g] = 1;
        }
        const auto base = "hy_gm" + std::to_string(it->first);
        if (sw.noglueperm == 0 && it->second.nodes.size() > 64u) {
            it->second.nodes = bank_aware_lane_order(it->second.nodes, it->second.nargs);
        }
        if (packed_idx && it->second.nargs == 8u) {
            // (The eight operand slots of a node side by side: ONE 16-byte table read per node instead of eight.)
            std::vector<std::uint32_t> v;
            for (const auto u : it->second.nodes) {
                const auto &args = p.nodes[u - n_eq].args;
                for (std::uint32_t a2 = 0; a2 < 8u; ++a2) {
                    v.push_back(a2 < args.size() ? static_cast<std::uint32_t>(pl.slot_of[args[a2].idx]) : n_slots + 1u);
                }
            }
            emit_utbl(base + "_p", v);
            packed_levels.insert(it->first);
        } else {
            for (std::uint32_t a2 = 0; a2 < it->second.nargs; ++a2) {
                std::vector<std::uint32_t> v;
                for (const auto u : it->second.nodes) {
                    const auto &args = p.nodes[u - n_eq].args;
                    v.push_back(a2 < args.size() ? static_cast<std::uint32_t>(pl.slot_of[args[a2].idx]) : n_slots + 1u);
                }
                emit_utbl(base + "_a" + std::to_string(a2), v);
            }
        }
        std::vector<std::uint32_t> v;
        for (const auto u : it->second.nodes) {
            v.push_back(static_cast<std::uint32_t>(pl.slot_of[u]));
        }
        emit_utbl(base + "_o", v);
        ++it;
    }
    // The same for the groups which stay on their own (<= 3 variable operands: operands and result in one 8-byte
    // record) and for the state-variable definitions (kind, slot, index of the input jet).
    if (packed_idx) {
        for (std::size_t g = 0; g < pl.groups.size(); ++g) {
            if (group_merged[g] != 0) {
                continue;
            }
            const auto &n0 = p.nodes[pl.groups[g].nodes[0] - n_eq];
            std::vector<std::size_t> va;
            for (std::size_t a = 0; a < n0.args.size(); ++a) {
                if (is_var(n0.args[a])) {
                    va.push_back(a);
                }
            }
            if (va.empty() || va.size() > 3u) {
                continue;
            }
            std::vector<std::uint32_t> v;
            for (const auto u : pl.groups[g].nodes) {
                for (std::size_t q = 0; q < 3u; ++q) {
                    v.push_back(q < va.size() ? static_cast<std::uint32_t>(pl.slot_of[p.nodes[u - n_eq].args[va[q]].idx]) : 0u);
                }
                v.push_back(static_cast<std::uint32_t>(pl.slot_of[u]));
            }
            emit_utbl("hy_g" + std::to_string(g) + "_q", v);
            q_groups.insert(g);
        }
        std::vector<std::uint32_t> v;
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            const auto &d = p.sv_defs[i];
            v.push_back(d.type == operand::kind::uvar ? 0u : (d.type == operand::kind::num ? 1u : 2u));
            v.push_back(d.type == operand::kind::uvar ? static_cast<std::uint32_t>(pl.slot_of[d.idx])
                                                      : (d.type == operand::kind::num ? 0u : d.idx));
            std::uint32_t ee = 0xffffu;
            for (std::uint32_t e2 = 0; e2 < n_ej; ++e2) {
                if (ej_slots[e2] == i) {
                    ee = e2;
                }
            }
            v.push_back(ee);
            v.push_back(0u);
        }
        emit_utbl("hy_sv_q", v);
    }
}

// The LAST glue level fused into the state recursion (orders >= 1): when every node of the level is a difference of
// two variables or a negation which only a state-variable definition reads (the accelerations of an N-body system
// with equal masses: sum over the later partners minus sum over the earlier ones), the lane of the state variable
// reads the two operands and subtracts itself - one barrier-separated phase per order less. Record per state
// variable: operand slots a, b (b: the zero slot when unused), operation (0 a - 0.0, 2 nothing: constant
// definition, 4 -a), index of the input jet. (Switch nofuse: A/B harness.)
void block_gen::pair_fused_last_level()
{
    fuse_last = packed_idx && sw.nofuse == 0 && pl.max_level >= 2u;
    std::vector<std::uint32_t> sv_f;
    if (fuse_last) {
        std::vector<char> read_elsewhere(p.nodes.size() + n_eq, 0);
        for (const auto &n : p.nodes) {
            for (const auto &o : n.args) {
                if (is_var(o)) {
                    read_elsewhere[o.idx] = 1;
                }
            }
        }
        for (const auto u : p.ev_u) {
            read_elsewhere[u] = 1;
        }
        std::map<std::uint32_t, std::uint32_t> n_defs;
        for (const auto &d : p.sv_defs) {
            if (d.type == operand::kind::uvar) {
                ++n_defs[d.idx];
            }
        }
        for (std::size_t g = 0; g < pl.groups.size() && fuse_last; ++g) {
            if (pl.groups[g].level != pl.max_level) {
                continue;
            }
            for (const auto u : pl.groups[g].nodes) {
                const auto &n = p.nodes[u - n_eq];
                const bool sub2 = n.kind == func_kind::sub && n.args.size() == 2u && is_var(n.args[0]) && is_var(n.args[1]);
                const bool neg = n.kind == func_kind::prod && n.args.size() == 2u && n.args[0].type == operand::kind::num
                                 && n.args[0].value == -1. && is_var(n.args[1]);
                fuse_last = fuse_last && (sub2 || neg) && read_elsewhere[u] == 0 && n_defs[u] == 1u;
            }
        }
    }
    if (fuse_last) {
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            const auto &d = p.sv_defs[i];
            std::uint32_t a = n_slots + 1u, b = n_slots + 1u, op = 2u, ee = 0xffffu;
            if (d.type == operand::kind::uvar) {
                op = 0u;
                a = static_cast<std::uint32_t>(pl.slot_of[d.idx]);
                if (d.idx >= n_eq && pl.lvl[d.idx] == pl.max_level && pl.cluster_of[d.idx] < 0) {
                    const auto &n = p.nodes[d.idx - n_eq];
                    if (n.kind == func_kind::sub) {
                        a = static_cast<std::uint32_t>(pl.slot_of[n.args[0].idx]);
                        b = static_cast<std::uint32_t>(pl.slot_of[n.args[1].idx]);
                    } else {
                        op = 4u;
                        a = static_cast<std::uint32_t>(pl.slot_of[n.args[1].idx]);
                    }
                }
            }
            for (std::uint32_t e2 = 0; e2 < n_ej; ++e2) {
                if (ej_slots[e2] == i) {
                    ee = e2;
                }
            }
            sv_f.insert(sv_f.end(), {a, b, op, ee});
        }
        emit_utbl("hy_sv_f", sv_f);
    }
    // One phase for the state recursion (with the fused level): a lane reads the operands of ITS definition - possibly
    // the slot of another state variable (x' = v) - and writes the next coefficient of its own variable; with the slots
    // of the state variables double-buffered by the parity of the order (bank 1 behind the slab) the write cannot
    // overtake another lane's read and the barrier between the two halves goes. Only when nothing but the state
    // recursion reads state-variable slots from the slab. MEASURED: nothing (1.647e6 with, 1.649e6 without): off; the switch dbuf switches it on.
    dbuf = fuse_last && sw.dbuf != 0;
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        dbuf = dbuf && ext_used[x] != 0;
    }
    for (std::size_t i = 0; i < p.nodes.size() && dbuf; ++i) {
        if (pl.cluster_of[n_eq + i] < 0) {
            for (const auto &o : p.nodes[i].args) {
                dbuf = dbuf && !(is_var(o) && o.idx < n_eq);
            }
        }
    }
}

// ---- stage 6d ----
// LDS copies of the index tables read at every order (cluster descriptors, glue operands / results, state-variable
// definitions), as far as they fit next to the slab and the input jets: a table lookup in front of every LDS access
// of the glue phases and of the head of a round is a ~1 us round trip to L2 per dependency level when it is a
// global load, ~0.1 us from LDS. Filled once per workgroup (the workgroups are persistent).
void block_gen::pair_lds_mirrors()
{
    std::uint64_t lds_used = (static_cast<std::uint64_t>(n_slots) + 2u + (dbuf ? n_eq : 0u)) * 8u + static_cast<std::uint64_t>(n_ej) * order * 8u
                             + 3u * 8u * (bs / 64u) + 64u;
    const std::uint64_t lds_cap = 160u * 1024u - 256u;
    std::ostringstream cp, defs;
    const auto mirror = [this, &lds_used, &cp, &defs](const std::string &name, std::size_t n, const char *type, std::uint64_t esz) {
        if (lds_used + n * esz + 8u > lds_cap) {
            return;
        }
        lds_used += (n * esz + 15u) / 16u * 16u;
        decl << "__shared__ " << type << " __attribute__((aligned(16))) l_" << name << "[" << n << "];\n";
        cp << "for (unsigned i_ = tid; i_ < " << n << "u; i_ += " << bs << "u) l_" << name << "[i_] = " << name
           << "[i_];\n";
        defs << "#define " << name << " l_" << name << "\n";
    };
    mirror("hy_dsc", static_cast<std::size_t>(n_dw) * nc, "unsigned", 4u);
    for (const auto &[name, n] : utbl_list) {
        bool unused = false;
        for (std::size_t g = 0; g < pl.groups.size(); ++g) {
            unused = unused || (group_merged[g] != 0 && name.rfind("hy_g" + std::to_string(g) + "_", 0) == 0);
            unused = unused || (q_groups.count(g) != 0u && name.rfind("hy_g" + std::to_string(g) + "_", 0) == 0
                                && name != "hy_g" + std::to_string(g) + "_q");
        }
        unused = unused || (packed_idx && (name == "hy_sv_kind" || name == "hy_sv_idx" || name == "hy_sv_ej"));
        if (!unused && (name.rfind("hy_g", 0) == 0 || name.rfind("hy_sv_", 0) == 0)) {
            mirror(name, n, "unsigned short", 2u);
        }
    }
    decl << cp.str() << "__syncthreads();\n" << defs.str();
}

// ---- stage 6e: order 0 - the node rules of the other modes -, its glue levels and the first state recursion ----
void block_gen::pair_order0()
{
    for (std::uint32_t r = 0; r < R; ++r) {
        for (std::uint32_t m = 0; m < M; ++m) {
            os << "double " << nm2("ca", m, r) << " = 0.0, " << nm2("cb", m, r) << " = 0.0;\n";
        }
        if (recip) {
            os << "double rca_" << r << " = 0.0;\n";
        }
    }

    os << "// ---- order 0 ----\n";
    for (std::uint32_t r = 0; r < R; ++r) {
        os << "{\n";
        desc_loads(r);
        unpack_ex(r);
        unpack_out(r);
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            e.val(pl.ext_u[0][x], 0) = e.def("HY_EJ(" + U(ej0b) + " + ex" + S(x) + ")");
        }
        for (const auto u : t0()) {
            e.node(u - n_eq, 0);
        }
        os << nm2("ca", 0, r) << " = " << e.val(t0()[pp.sq], 0) << ";\n";
        os << nm2("cb", 0, r) << " = " << e.val(t0()[pp.pw], 0) << ";\n";
        if (recip) {
            os << "rca_" << r << " = 1.0 / " << nm2("ca", 0, r) << ";\n";
        }
        const std::string v[3] = {e.val(t0()[pp.pr[0]], 0), e.val(t0()[pp.pr[1]], 0), e.val(t0()[pp.pr[2]], 0)};
        store_out(v);
        os << "}\n";
    }
    pair_glue_levels(0);
    pair_recursion(false);
}

// ---- stage 6f: the glue levels of order 0 (k = 0) or of the orders inside the loop ----
// The glue groups of a dependency level, STAGED: the nodes of a level do not read each other, but the compiler
// cannot know that the slab store of one block does not alias the slab loads of the next one - emitted block by block
// (index lookup, operands, sum, store) a level is one chain of ~40 dependent LDS round trips on the single wavefront
// of a SIMD. Here: all the index lookups of the level, then all the operand loads, then the arithmetic, then the
// stores.
void block_gen::pair_glue_level_staged(std::uint32_t lev, std::uint32_t k)
{
    std::string st_idx, st_ld, st_ar, st_wr;
    const auto before = take_os();
    if (const auto mit = merged.find(lev); mit != merged.end() && !(exp_mode == 2 && k != 0u)) {
        const auto &m = mit->second;
        const auto gn = "hy_gm" + std::to_string(lev);
        const auto ng = static_cast<std::uint32_t>(m.nodes.size());
        for (std::uint32_t r = 0; r * bs < ng; ++r) {
            const auto tag = "_m" + std::to_string(lev) + "_" + std::to_string(r) + "_" + std::to_string(k == 0u ? 0 : 1);
            const bool partial = (r + 1u) * bs > ng;
            const auto inside = "(tid + " + std::to_string(r * bs) + "u < " + std::to_string(ng) + "u)";
            os << "const unsigned j" << tag << " = "
               << (partial ? inside + " ? tid + " + std::to_string(r * bs) + "u : " + std::to_string(ng - 1u) + "u"
                           : "tid + " + std::to_string(r * bs) + "u")
               << ";\n";
            if (packed_levels.count(lev) != 0u) {
                os << "const hy_u4 iw" << tag << " = *(const hy_u4 *)(" << gn << "_p + 8u * j" << tag << ");\n";
                for (std::uint32_t a2 = 0; a2 < 8u; ++a2) {
                    os << "const unsigned ia" << a2 << tag << " = " << ((a2 & 1u) != 0u ? "(iw" + tag + "[" + std::to_string(a2 / 2u) + "] >> 16)"
                                                                                   : "(iw" + tag + "[" + std::to_string(a2 / 2u) + "] & 0xffffu)")
                       << ";\n";
                }
            } else {
                for (std::uint32_t a2 = 0; a2 < m.nargs; ++a2) {
                    os << "const unsigned ia" << a2 << tag << " = " << gn << "_a" << a2 << "[j" << tag << "];\n";
                }
            }
            os << "const unsigned io" << tag << " = "
               << (partial ? inside + " ? (unsigned)" + gn + "_o[j" + tag + "] : " + std::to_string(n_slots) + "u"
                           : "(unsigned)" + gn + "_o[j" + tag + "]")
               << ";\n";
            st_idx += take_os();
            std::vector<std::string> terms;
            for (std::uint32_t a2 = 0; a2 < m.nargs; ++a2) {
                terms.push_back(e.def("slab[ia" + std::to_string(a2) + tag + "]"));
            }
            st_ld += take_os();
            const auto res = e.pairwise_sum(std::move(terms));
            st_ar += take_os();
            st_wr += "slab[io" + tag + "] = " + res + ";\n";
        }
    }
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &grp = pl.groups[g];
        if (grp.level != lev || group_merged[g] != 0 || (exp_mode == 2 && k != 0u)) {
            continue;
        }
        const auto rep = grp.nodes[0];
        const auto &n0 = p.nodes[rep - n_eq];
        const auto gn = "hy_g" + std::to_string(g);
        const auto ng = static_cast<std::uint32_t>(grp.nodes.size());
        for (std::uint32_t r = 0; r * bs < ng; ++r) {
            const auto tag = "_" + std::to_string(g) + "_" + std::to_string(r) + "_" + std::to_string(k == 0u ? 0 : 1);
            const bool partial = (r + 1u) * bs > ng;
            os << "const unsigned j" << tag << " = ";
            if (partial) {
                os << "(tid + " << r * bs << "u < " << ng << "u) ? tid + " << r * bs << "u : " << ng - 1u << "u;\n";
            } else {
                os << "tid + " << r * bs << "u;\n";
            }
            if (q_groups.count(g) != 0u) {
                os << "const hy_u2 iq" << tag << " = *(const hy_u2 *)(" << gn << "_q + 4u * j" << tag << ");\n";
                std::uint32_t q = 0;
                for (std::size_t a = 0; a < n0.args.size(); ++a) {
                    if (is_var(n0.args[a])) {
                        os << "const unsigned ia" << a << tag << " = "
                           << (q == 0u ? "(iq" + tag + "[0] & 0xffffu)" : (q == 1u ? "(iq" + tag + "[0] >> 16)" : "(iq" + tag + "[1] & 0xffffu)"))
                           << ";\n";
                        ++q;
                    }
                }
                os << "const unsigned io" << tag << " = "
                   << (partial ? "(tid + " + std::to_string(r * bs) + "u < " + std::to_string(ng) + "u) ? (iq" + tag + "[1] >> 16) : "
                                     + std::to_string(n_slots) + "u"
                               : "(iq" + tag + "[1] >> 16)")
                   << ";\n";
            } else {
                for (std::size_t a = 0; a < n0.args.size(); ++a) {
                    if (is_var(n0.args[a])) {
                        os << "const unsigned ia" << a << tag << " = " << gn << "_a" << a << "[j" << tag << "];\n";
                    }
                }
                os << "const unsigned io" << tag << " = "
                   << (partial ? "(tid + " + std::to_string(r * bs) + "u < " + std::to_string(ng) + "u) ? (unsigned)" + gn
                                     + "_o[j" + tag + "] : " + std::to_string(n_slots) + "u"
                               : "(unsigned)" + gn + "_o[j" + tag + "]")
                   << ";\n";
            }
            st_idx += take_os();
            const auto saved = e.numpar_override;
            std::vector<std::pair<std::uint32_t, std::string>> saved_vals;
            for (std::size_t a = 0; a < n0.args.size(); ++a) {
                const auto &o = n0.args[a];
                if (is_var(o)) {
                    const auto nm_ = e.def(exp_mode == 5 ? "slab[(ia" + std::to_string(a) + tag + " & 1u) + tid + "
                                                               + std::to_string(a * 2u) + "u]"
                                                         : "slab[ia" + std::to_string(a) + tag + "]");
                    saved_vals.emplace_back(o.idx, e.val(o.idx, k));
                    e.val(o.idx, k) = nm_;
                } else if (o.type == operand::kind::num) {
                    e.numpar_override[&o] = gn + "_a" + std::to_string(a) + "[j" + tag + "]";
                }
            }
            st_ld += take_os();
            if (n0.kind == func_kind::prod && n0.args[0].type == operand::kind::num && n0.args[0].value == -1.) {
                e.numpar_override.erase(&n0.args[0]);
            }
            e.node(rep - n_eq, k);
            st_ar += take_os();
            st_wr += "slab[io" + tag + "] = " + e.val(rep, k) + ";\n";
            for (auto it = saved_vals.rbegin(); it != saved_vals.rend(); ++it) {
                e.val(it->first, k) = it->second;
            }
            e.numpar_override = saved;
        }
    }
    os << before << "{\n" << st_idx << st_ld << st_ar << st_wr << "}\n";
}

void block_gen::pair_glue_levels(std::uint32_t k)
{
    for (std::uint32_t lev = 1; lev <= pl.max_level; ++lev) {
        if (k != 0u && fuse_last && lev == pl.max_level) {
            continue; // (computed by the lanes of the state variables, pair_recursion())
        }
        pair_glue_level_staged(lev, k);
        sync();
    }
}

// ---- stage 6g ----
// State-variable recursion (src/taylor_02.cpp:245-287) with the order-(k + 1) values of the external inputs
// recorded in LDS. dyn: k is the loop variable.
void block_gen::pair_recursion(bool dyn)
{
    os << "{\n";
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        os << "double xn" << r << " = 0.0;\nunsigned svej" << r << " = 0xffffu;\n";
        os << "{ const unsigned i = tid + " << r * bs << "u; if (i < " << n_eq << "u) {\n";
        if (dyn && fuse_last) {
            os << "const hy_u2 svf = *(const hy_u2 *)(hy_sv_f + 4u * i);\n";
            os << "svej" << r << " = svf[1] >> 16;\n";
            os << "const unsigned op_ = svf[1] & 0xffffu;\n";
            if (dbuf) {
                // (Order-k coefficients of the state variables: bank (k - 1) & 1; the new ones go to bank k & 1.)
                os << "const unsigned rbo = ((k - 1u) & 1u) * " << U(n_slots + 2u) << ";\n";
                os << "const unsigned sa_ = svf[0] & 0xffffu, sb_ = svf[0] >> 16;\n";
                os << "const double xa_ = slab[sa_ + (sa_ < " << n_eq << "u ? rbo : 0u)], xb_ = slab[sb_ + (sb_ < " << n_eq
                   << "u ? rbo : 0u)];\n";
            } else {
                os << "const double xa_ = slab[svf[0] & 0xffffu], xb_ = slab[svf[0] >> 16];\n";
            }
            os << "const double xv = op_ == 4u ? -xa_ : xa_ - xb_;\n";
            if (recip) {
                os << "const double xq = xv * rkd1;\n";
                os << "xn" << r << " = op_ == 2u ? 0.0 : __builtin_fma(__builtin_fma(-xq, kd + 1.0, xv), rkd1, xq);\n";
            } else {
                os << "xn" << r << " = op_ == 2u ? 0.0 : xv / (kd + 1.0);\n";
            }
            os << "} }\n";
            continue;
        }
        if (packed_idx) {
            os << "const hy_u2 svq = *(const hy_u2 *)(hy_sv_q + 4u * i);\n";
            os << "svej" << r << " = svq[1] & 0xffffu;\n";
            os << "const unsigned kd_ = svq[0] & 0xffffu, svi_ = svq[0] >> 16;\n";
        } else {
            os << "const unsigned kd_ = hy_sv_kind[i], svi_ = hy_sv_idx[i];\n";
        }
        if (dyn) {
            if (recip) {
                os << "if (kd_ == 0u) { const double xv = slab[svi_], xq = xv * rkd1; xn" << r
                   << " = __builtin_fma(__builtin_fma(-xq, kd + 1.0, xv), rkd1, xq); }\n";
            } else {
                os << "if (kd_ == 0u) xn" << r << " = slab[svi_] / (kd + 1.0);\n";
            }
        } else {
            os << "if (kd_ == 0u) xn" << r << " = slab[svi_];\n";
            os << "else if (kd_ == 1u) xn" << r << " = hy_sv_val[i];\n";
            os << "else xn" << r << " = a.pars[(u64)svi_ * N + s];\n";
        }
        os << "} }\n";
    }
    if (!(dyn && dbuf)) {
        sync();
    }
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        os << "{ const unsigned i = tid + " << r * bs << "u; if (i < " << n_eq << "u) {\n";
        if (dyn && dbuf) {
            os << "slab[i + (k & 1u) * " << U(n_slots + 2u) << "] = xn" << r << ";\n";
        } else {
            os << "slab[i] = xn" << r << ";\n";
        }
        if (dyn) {
            os << "sjet[(k + 1u) * " << n_eq << "u + i] = xn" << r << ";\n";
            os << "const unsigned ee = " << (packed_idx ? "svej" + std::to_string(r) : std::string("hy_sv_ej[i]")) << ";\n";
            os << "if (ee != 0xffffu && k + 1u < " << P << "u) HY_EJW((" << P - 2u << "u - k) * " << U(ejrow)
               << " + ee * 8u) = xn" << r << ";\n";
            os << "if (k + 1u == " << P << "u) mo = hy_max(mo, fabs(xn" << r << "));\n";
            os << "else if (k + 2u == " << P << "u) mom1 = hy_max(mom1, fabs(xn" << r << "));\n";
        } else {
            os << "sjet[" << n_eq << "u + i] = xn" << r << ";\n";
            os << "const unsigned ee = " << (packed_idx ? "svej" + std::to_string(r) : std::string("hy_sv_ej[i]")) << ";\n";
            os << "if (ee != 0xffffu) HY_EJW(" << U(static_cast<std::uint64_t>(P - 2u) * ejrow) << " + ee * 8u) = xn" << r
               << ";\n";
        }
        os << "} }\n";
    }
    sync();
    os << "}\n";
}

// ---- stage 6h: orders 1 .. P - 1 ----
// Tape registers of slot 1 (set 1 of the pipeline): slot 1 pairs order 1 with order k - 1, whose coefficients the lane
// computed itself one order earlier - they are handed over in registers (no load: the head of a group does not
// wait for the memory system). NOTE: loading them back right behind their stores is NOT an option: under load
// such a load was observed to overtake the store (stale values, runaway step sizes).
// (Rounds per group G, depth D of the tape-load pipeline, cross-group prefetch, hand-over: pair_resolve_pipeline().)
void block_gen::pair_order_loop()
{
    if (xpf) {
        for (std::uint32_t i = 2; i <= D + 1u; ++i) {
            for (std::uint32_t q = 0; q < G; ++q) {
                os << "double " << xname("xa", i, q) << " = 0.0, " << xname("xb", i, q) << " = 0.0;\n";
            }
        }
    }
    for (std::uint32_t r = 0; r < R; ++r) {
        os << "double ap1_" << r << " = 0.0, bp1_" << r << " = 0.0;\n";
        for (std::uint32_t h = 2; h <= hand; ++h) {
            os << "double ah" << h << "_" << r << " = 0.0, bh" << h << "_" << r << " = 0.0;\n";
        }
    }
    if (hoist) {
        for (std::uint32_t r = 0; r < R; ++r) {
            desc_loads(r);
        }
    }
    if (keepdz) {
        for (std::uint32_t r = 0; r < R; ++r) {
            for (std::uint32_t c = 0; c < 3u; ++c) {
                os << "double hdz" << c << "_" << r << ";\n";
            }
            os << "{\n";
            if (!hoist) {
                desc_loads(r);
            }
            unpack_ex(r);
            for (std::uint32_t c = 0; c < 3u; ++c) {
                os << "hdz" << c << "_" << r << " = HY_EJ(" << U(ej0b) << " + ex" << pp.de[c][0] << ") - HY_EJ(" << U(ej0b) << " + ex"
                   << pp.de[c][1] << ");\n";
            }
            os << "}\n";
        }
    }
    os << "#pragma nounroll\nfor (unsigned k = 1; k < " << P << "u; ++k) {\n";
    os << "const double kd = (double)k;\n";
    os << "const double c0k = kd * " << fp_literal(ex) << ";\n";
    if (recip) {
        os << "const double rkd = 1.0 / kd, rkd1 = 1.0 / (kd + 1.0);\n";
    }
    os << "const unsigned nm1 = k >> 1;\nconst bool even = (k & 1u) == 0u;\n";
    os << "const unsigned kbr = (" << P - 1u << "u - k) * " << U(ejrow) << ";\n";
    if (il_tape) {
        os << "const unsigned tpa = k * " << 2u * rowb << "u;\n";
    } else {
        os << "const unsigned tpa = (" << arow0 << "u + k) * " << rowb << "u;\n";
        os << "const unsigned tpb = (" << brow0 << "u + k) * " << rowb << "u;\n";
    }
    for (std::uint32_t r0 = 0, gi = 0; r0 < R; r0 += G, ++gi) {
        pair_group(r0, std::min(R, r0 + G), gi);
    }
    pair_glue_levels(1);
    pair_recursion(true);
    os << "}\n";
}

// The LDS reads of step (i, r) into set `set`.
void block_gen::lds_step(std::uint32_t i, std::uint32_t r, std::uint32_t set)
{
    if (exp_mode == 3 || exp_mode == 34) {
        for (std::uint32_t c = 0; c < 3u; ++c) {
            for (std::uint32_t side = 0; side < 2u; ++side) {
                os << raw(set, 0, c, side) << " = kd;\n" << raw(set, 1, c, side) << " = c0k;\n";
            }
        }
        return;
    }
    // (eo*_r: byte offsets of the inputs of the lane's cluster of round r inside a row; kx*_r: the same plus the row of
    // order k - one register each for the duration of a group, so that every read is "register + constant".)
    for (std::uint32_t c = 0; c < 3u; ++c) {
        for (std::uint32_t side = 0; side < 2u; ++side) {
            os << raw(set, 0, c, side) << " = HY_EJ(eo" << pp.de[c][side] << "_" << r << " + "
               << U(static_cast<std::uint64_t>(P - 1u - i) * ejrow) << ");\n";
            os << raw(set, 1, c, side) << " = HY_EJ(kx" << pp.de[c][side] << "_" << r << " + "
               << U(static_cast<std::uint64_t>(i) * ejrow) << ");\n";
        }
    }
}

// The tape loads of slot i (rounds r0 .. r1 - 1) into the set i % (D + 1).
void block_gen::tape_loads(std::uint32_t i, std::uint32_t r0, std::uint32_t r1)
{
    const bool skip_high = i >= 2u && i <= hand;
    if (skip_high && i < M) {
        return;
    }
    const auto back = "(nm1 < " + S(i) + "u ? nm1 : " + S(i) + "u) * " + std::to_string(rowb) + "u";
    const auto own = "(k < " + S(i) + "u ? k : " + S(i) + "u) * " + std::to_string(rowb) + "u";
    if (exp_mode == 4 || exp_mode == 34) {
        for (std::uint32_t r = r0; r < r1; ++r) {
            os << gname("ap", i, r) << " = kd;\n" << gname("bp", i, r) << " = c0k;\n";
            if (i >= M) {
                os << gname("al", i, r) << " = kd;\n" << gname("bl", i, r) << " = c0k;\n";
            }
        }
        return;
    }
    // (reg_high: no request while the high member of the slot is a row in registers.)
    os << (reg_high && i < M ? "if (k >= " + S(i + M) + "u) {\n" : std::string("{\n"));
    if (il_tape) {
        os << "const unsigned sa = tpa - 2u * " << back << ";\n";
        if (i >= M) {
            os << "const unsigned oa = 2u * " << own << ";\n";
        }
        for (std::uint32_t r = r0; r < r1; ++r) {
            if (!skip_high) {
                os << "{ const hy_dd2 t_ = HY_TLD2(2u * lo_" << r << ", sa); " << gname("ap", i, r) << " = t_[0]; "
                   << gname("bp", i, r) << " = t_[1]; }\n";
            }
            if (i >= M) {
                os << "{ const hy_dd2 t_ = HY_TLD2(2u * lo_" << r << ", oa); " << gname("al", i, r) << " = t_[0]; "
                   << gname("bl", i, r) << " = t_[1]; }\n";
            }
        }
        os << "}\n";
        return;
    }
    os << "const unsigned sa = tpa - " << back << ", sb = tpb - " << back << ";\n";
    if (i >= M) {
        os << "const unsigned oa = " << arow0 * rowb << "u + " << own << ", ob = " << brow0 * rowb << "u + " << own << ";\n";
    }
    for (std::uint32_t r = r0; r < r1; ++r) {
        os << gname("ap", i, r) << " = HY_TLD(lo_" << r << ", sa);\n";
        os << gname("bp", i, r) << " = HY_TLD(lo_" << r << ", sb);\n";
        if (i >= M) {
            os << gname("al", i, r) << " = HY_TLD(lo_" << r << ", oa);\n";
            os << gname("bl", i, r) << " = HY_TLD(lo_" << r << ", ob);\n";
        }
    }
    os << "}\n";
}

// The cluster phase of order k for the rounds r0 .. r1 - 1 of the lane (group gi), SLOT-major: for slot i = 1 ..
// floor(k / 2) (early exit after the last one) the rounds of the group, with the five accumulators of every round in
// registers. One software pipeline runs through the whole (slot, round) sequence of an order:
//  * tape loads: those of slot i + 1 (all rounds) are issued, unconditionally, at the head of slot i - rows of
//    slots beyond the last one are clamped to rows which are loaded anyway (L1 hits) -, so that an order pays the
//    latency of the memory system once (slot 1) and not once per round;
//  * LDS reads: the 12 raw values of a step are read before the arithmetic of the previous step (two sets,
//    ping-pong): with ONE wavefront per SIMD nothing else covers the LDS latency.
void block_gen::pair_group(std::uint32_t r0, std::uint32_t r1, std::uint32_t gi)
{
    const auto Rg = r1 - r0;
    const bool hand2 = hand >= 2u;
    const auto step_set = [this, Rg, r0](std::uint32_t i, std::uint32_t r) { return nopp ? 0u : ((i - 1u) * Rg + (r - r0)) % 2u; };
    os << "{\n";
    // Declarations of the pipeline registers.
    for (std::uint32_t set = 0; set <= D; ++set) {
        for (std::uint32_t r = r0; r < r1; ++r) {
            std::string d;
            if (set != 1u) {
                d = "ap" + S(set) + "_" + S(r) + " = 0.0, bp" + S(set) + "_" + S(r) + " = 0.0";
            }
            if (M < T) {
                d += std::string(d.empty() ? "" : ", ") + "al" + S(set) + "_" + S(r) + " = 0.0, bl" + S(set) + "_" + S(r)
                     + " = 0.0";
            }
            if (!d.empty()) {
                os << "double " << d << ";\n";
            }
        }
    }
    for (std::uint32_t set = 0; set < 2u; ++set) {
        for (std::uint32_t c = 0; c < 3u; ++c) {
            for (std::uint32_t side = 0; side < 2u; ++side) {
                os << "double " << raw(set, 0, c, side) << " = 0.0, " << raw(set, 1, c, side) << " = 0.0;\n";
            }
        }
    }
    // Head: descriptors, the tape loads of slot 1, slot 0 (order-k differences x order-0 ones).
    for (std::uint32_t r = r0; r < r1; ++r) {
        if (!hoist) {
            desc_loads(r);
        }
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            // (The optimiser re-derives these from the packed word where they are used - one SDWA addition per read
            // of a dynamic row; pinning them in registers was measured: they end up in AGPRs and every read pays a
            // copy instead.)
            os << "const unsigned eo" << x << "_" << r << " = " << ex_expr(x, r) << ";\n";
            os << "const unsigned kx" << x << "_" << r << " = kbr + eo" << x << "_" << r << ";\n";
        }
    }
    if (!xpf) {
        for (std::uint32_t i = 2; i <= D && i < T; ++i) {
            tape_loads(i, r0, r1);
        }
    }
    if (hand2) {
        for (std::uint32_t r = r0; r < r1; ++r) {
            os << "const double ah1s_" << r << " = ap1_" << r << ", bh1s_" << r << " = bp1_" << r << ";\n";
        }
    }
    for (std::uint32_t r = r0; r < r1; ++r) {
        os << "double ssq_" << r << ", spw_" << r << " = 0.0, sf0_" << r << ", sf1_" << r << ", sf2_" << r << ";\n";
        os << "{\n";
        unpack_ex(r);
        for (std::uint32_t c = 0; c < 3u; ++c) {
            diff("dk" + S(c), c, "kbr");
            if (keepdz) {
                os << "const double dz" << c << " = hdz" << c << "_" << r << ";\n";
            } else {
                diff("dz" + S(c), c, U(ej0b));
            }
        }
        os << "ssq_" << r << " = dz0 * dk0;\nssq_" << r << " = __builtin_fma(dz1, dk1, ssq_" << r << ");\nssq_" << r
           << " = __builtin_fma(dz2, dk2, ssq_" << r << ");\n";
        for (std::uint32_t c = 0; c < 3u; ++c) {
            os << "sf" << c << "_" << r << " = dk" << c << " * " << nm2("cb", 0, r) << ";\n";
        }
        os << "}\n";
    }
    if (T > 1u) {
        if (!nopp) {
            lds_step(1, r0, step_set(1, r0));
            os << "__builtin_amdgcn_sched_barrier(0);\n";
        }
        os << (exp_mode == 1 ? "if (nm1 > 1000u) {\n" : "if (nm1 != 0u) {\n");
        for (std::uint32_t i = 1; i < T; ++i) {
            os << "{\n";
            if (i + D < T && !(xpf && i + D <= D + 1u)) {
                tape_loads(i + D, r0, r1);
            }
            // Weights of the last slot of an even order (middle term): 1/2 on the squares, 0 on the mirrored
            // products; scalar factors k a - j (a + 1) of the terms j = i and j = p = k - i.
            os << "const bool mid = even & (nm1 == " << i << "u);\n";
            os << "const double wq = mid ? 0.5 : 1.0, w2 = mid ? 0.0 : 1.0;\n";
            os << "const double ci = c0k - " << fp_literal(static_cast<double>(i) * e1) << ";\n";
            os << "const double cp = c0k - (kd - " << fp_literal(static_cast<double>(i)) << ") * " << fp_literal(e1)
               << ";\n";
            if (reg_high_br && i >= 2u && i < M) {
                os << "if (k < " << S(i + M) << "u) {\n";
                for (std::uint32_t r = r0; r < r1; ++r) {
                    std::string a = nm2("ca", M - 1u, r), b = nm2("cb", M - 1u, r);
                    for (std::uint32_t m = M - 1u; m-- > i;) {
                        a = "(k == " + S(i + m) + "u ? " + nm2("ca", m, r) + " : " + a + ")";
                        b = "(k == " + S(i + m) + "u ? " + nm2("cb", m, r) + " : " + b + ")";
                    }
                    os << gname("ap", i, r) << " = " << a << ";\n" << gname("bp", i, r) << " = " << b << ";\n";
                }
                os << "}\n";
            }
            for (std::uint32_t r = r0; r < r1; ++r) {
                const auto set = step_set(i, r);
                os << "{\n";
                if (nopp) {
                    lds_step(i, r, 0u);
                } else {
                    if (r + 1u < r1) {
                        lds_step(i, r + 1u, 1u - set);
                    } else if (i + 1u < T) {
                        lds_step(i + 1u, r0, 1u - set);
                    }
                    os << "__builtin_amdgcn_sched_barrier(0);\n";
                }
                for (std::uint32_t c = 0; c < 3u; ++c) {
                    os << "const double pi" << c << " = " << raw(set, 0, c, 0) << " - " << raw(set, 0, c, 1) << ";\n";
                    os << "const double pp" << c << " = " << raw(set, 1, c, 0) << " - " << raw(set, 1, c, 1) << ";\n";
                }
                const auto ai = i < M ? nm2("ca", i, r) : gname("al", i, r);
                const auto bi = i < M ? nm2("cb", i, r) : gname("bl", i, r);
                auto aph = gname("ap", i, r), bph = gname("bp", i, r);
                if (xpf && i >= 2u && i <= D + 1u) {
                    aph = xname("xa", i, r - r0);
                    bph = xname("xb", i, r - r0);
                }
                if (i >= 2u && i <= hand) {
                    aph = "ah" + S(i) + "_" + S(r);
                    bph = "bh" + S(i) + "_" + S(r);
                }
                if (reg_high && !reg_high_br && i >= 2u && i < M) {
                    // (k - i = m < M: the register copy of row m.)
                    for (std::uint32_t m = i; m < M; ++m) {
                        aph = "(k == " + S(i + m) + "u ? " + nm2("ca", m, r) + " : " + aph + ")";
                        bph = "(k == " + S(i + m) + "u ? " + nm2("cb", m, r) + " : " + bph + ")";
                    }
                    os << "const double aph = " << aph << ", bph = " << bph << ";\n";
                    aph = "aph";
                    bph = "bph";
                }
                os << "const double bpw = " << bph << " * w2;\n";
                os << "double sqt = pi0 * pp0;\nsqt = __builtin_fma(pi1, pp1, sqt);\nsqt = __builtin_fma(pi2, pp2, sqt);\n";
                os << "ssq_" << r << " = __builtin_fma(wq, sqt, ssq_" << r << ");\n";
                os << "spw_" << r << " = __builtin_fma(ci, " << aph << " * " << bi << ", spw_" << r << ");\n";
                os << "spw_" << r << " = __builtin_fma(cp, " << ai << " * bpw, spw_" << r << ");\n";
                for (std::uint32_t c = 0; c < 3u; ++c) {
                    os << "sf" << c << "_" << r << " = __builtin_fma(pp" << c << ", " << bi << ", sf" << c << "_" << r
                       << ");\n";
                    os << "sf" << c << "_" << r << " = __builtin_fma(pi" << c << ", bpw, sf" << c << "_" << r << ");\n";
                }
                os << "}\n";
            }
            if (i + 1u < T) {
                os << "if (nm1 == " << i << "u) goto hy_done_" << gi << ";\n";
            }
            os << "}\n";
        }
        os << "}\nhy_done_" << gi << ":;\n";
        if (xpf) {
            pair_group_prefetch(r1);
        }
    }
    pair_group_finish(r0, r1);
    os << "}\n";
}

// Cross-group prefetch: the requests for the next group of this order, or for the first group of the next order: rows
// k' - min(floor(k' / 2), i).
void block_gen::pair_group_prefetch(std::uint32_t r1)
{
    const bool last = r1 >= R;
    const auto n0 = last ? 0u : r1;
    os << (last ? "if (k + 1u < " + S(P) + "u) {\nconst unsigned kn = k + 1u, tan = tpa + " + U(rowb) + ", tbn = tpb + " + U(rowb) + ";\n"
                : std::string("{\nconst unsigned kn = k, tan = tpa, tbn = tpb;\n"));
    os << "const unsigned nmn = kn >> 1;\n";
    for (std::uint32_t q = 0; q < G; ++q) {
        os << "unsigned xcl" << q << " = " << cl_expr(n0 + q) << ";\nasm volatile(\"\" : \"+v\"(xcl" << q << "));\n";
        os << "const unsigned xlo" << q << " = xcl" << q << " * 8u;\n";
    }
    for (std::uint32_t i = 2; i <= D + 1u; ++i) {
        os << "{\nconst unsigned bk_ = (nmn < " << i << "u ? nmn : " << i << "u) * " << U(rowb) << ";\n";
        for (std::uint32_t q = 0; q < G; ++q) {
            os << xname("xa", i, q) << " = HY_TLD(xlo" << q << ", tan - bk_);\n";
            os << xname("xb", i, q) << " = HY_TLD(xlo" << q << ", tbn - bk_);\n";
        }
        os << "}\n";
    }
    os << "}\n";
}

// Slot 0, second half, and the quotient of the pow recurrence (src/math/pow.cpp:546-549); stores; the register
// copies of the coefficients of order < M.
void block_gen::pair_group_finish(std::uint32_t r0, std::uint32_t r1)
{
    const bool hand2 = hand >= 2u;
    for (std::uint32_t r = r0; r < r1; ++r) {
        os << "{\n";
        unpack_ex(r);
        unpack_out(r);
        for (std::uint32_t c = 0; c < 3u; ++c) {
            if (keepdz) {
                os << "const double dz" << c << " = hdz" << c << "_" << r << ";\n";
            } else {
                diff("dz" + S(c), c, U(ej0b));
            }
        }
        os << "const double ak = ssq_" << r << " + ssq_" << r << ";\n";
        os << "const double spw = __builtin_fma(c0k, ak * " << nm2("cb", 0, r) << ", spw_" << r << ");\n";
        if (recip) {
            // (The quotient of the recurrence as a product with RN(1 / r2^[0]) RN(1 / k) and one correction with the
            // exact residual: 5 operations instead of the ~13 of a division, correctly rounded but for rare ties.)
            os << "const double rinv = rca_" << r << " * rkd, den = kd * " << nm2("ca", 0, r) << ";\n";
            os << "const double bq = spw * rinv;\n";
            os << "const double bk = __builtin_fma(__builtin_fma(-bq, den, spw), rinv, bq);\n";
        } else {
            os << "const double bk = spw / (kd * " << nm2("ca", 0, r) << ");\n";
        }
        for (std::uint32_t c = 0; c < 3u; ++c) {
            os << "const double sf" << c << " = __builtin_fma(dz" << c << ", bk, sf" << c << "_" << r << ");\n";
        }
        // (Row k is read from the tape by a slot i > hand of an order k + i <= P - 1 with i <= k: rows beyond P - 2 - hand
        // are only ever handed over in registers; a row below min(M, hand + 1) is never read from the tape either - as a
        // low member it is in registers, as a high member it belongs to a slot i <= hand.)
        os << (reg_high ? "if (k >= " + S(M) + "u && k + 2u < " + S(P) + "u) {\n" : "if (k >= " + S(std::min(M, hand + 1u)) + "u && k + " + S(hand + 1u) + "u < " + S(P) + "u) {\n");
        if (il_tape) {
            os << "HY_TST2(ak, bk, 2u * lo_" << r << ", tpa);\n";
        } else {
            os << "HY_TST(ak, lo_" << r << ", tpa);\nHY_TST(bk, lo_" << r << ", tpb);\n";
        }
        os << "}\n";
        const std::string v[3] = {"sf0", "sf1", "sf2"};
        store_out(v);
        for (std::uint32_t h = hand; h >= 3u; --h) {
            os << "ah" << h << "_" << r << " = ah" << h - 1u << "_" << r << ";\nbh" << h << "_" << r << " = bh" << h - 1u << "_" << r
               << ";\n";
        }
        if (hand2) {
            os << "ah2_" << r << " = ah1s_" << r << ";\nbh2_" << r << " = bh1s_" << r << ";\n";
        }
        os << "ap1_" << r << " = ak;\nbp1_" << r << " = bk;\n";
        if (M > 1u) {
            os << "if (k < " << M << "u) {\n";
            for (std::uint32_t m = 1; m < M; ++m) {
                os << nm2("ca", m, r) << " = (k == " << m << "u) ? ak : " << nm2("ca", m, r) << ";\n";
                os << nm2("cb", m, r) << " = (k == " << m << "u) ? bk : " << nm2("cb", m, r) << ";\n";
            }
            os << "}\n";
        }
        os << "}\n";
    }
}

} // namespace heyoka_amd::block_detail
