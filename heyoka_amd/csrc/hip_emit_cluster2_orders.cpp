// Cluster code generation, version 2 (hip_emit_cluster2_gen.hpp): emission helpers, the order programs of the three kernels
// and the helpers of the module text. The SSA names they hand out depend on the order of the calls.
#include <cstdio>

#include "hip_emit_cluster2_gen.hpp"

namespace heyoka_amd::cluster2_detail
{

// ---- 4. Emission helpers. ----
std::string cluster2_gen::slabk(std::uint32_t k, const std::string &tbl) const
{
    // Parity buffer of order k.
    return (k % 2u == 0u || buf_stride == 0u) ? ("slab[" + tbl + "]")
                                              : ("slab[" + tbl + " + " + std::to_string(buf_stride) + "u]");
}

// Owner-slot bookkeeping when a new coefficient of a state variable is produced.
void cluster2_gen::publish_sv(owner_slot &ow, std::uint32_t k, const std::string &name)
{
    ow.xname[k] = name;
    if (ow.slab_needed) {
        os << slabk(k, utname(ow.out_tbl)) << " = " << name << ";\n";
    }
    if (k != 0u && !ow.derived) {
        // (The order-0 row of the jets *is* the current state: written by the update of the previous step.)
        os << jet_at(k, ow.col) << " = " << name << ";\n";
    }
    // NOTE: the idle lanes of a partially filled slot hold a copy of a valid lane's coefficient: harmless in a maximum.
    const char *acc = (k == 0u) ? "m0" : (k == order ? "mo" : (k == order - 1u ? "mom1" : nullptr));
    if (acc != nullptr && ow.reduced && k != 0u) {
        // (Lane-reduced round: the lanes without a sum hold partial sums, which stay out of the norms - a select at the
        // two orders which enter them.)
        os << acc << " = hy_nmax(" << acc << ", fabs(ovalid" << ow.col << " ? " << name << " : 0.0));\n";
    } else if (acc != nullptr) {
        os << acc << " = hy_nmax(" << acc << ", fabs(" << name << "));\n";
    }
}

// A 16-byte LDS read of two adjacent slots (wide-read layout: the table entries are even, the slab is 16-byte aligned).
std::string cluster2_gen::wide_read(const std::string &tbl)
{
    const auto nm = "w" + std::to_string(n_wide++);
    os << "const hy_d2 " << nm << " = *reinterpret_cast<const hy_d2 *>(slab + " << tbl << ");\n";
    ++e.n_stmt;
    return nm;
}

// A glue round is emitted in two halves: the LDS reads of the operands, and the computation (node rule,
// export, fused state-variable recursions). In overlap mode independent FMA work is placed in between.
std::vector<std::string> cluster2_gen::emit_glue_reads(std::size_t g, std::uint32_t r, std::uint32_t k)
{
    const auto &grp = pl.groups[g];
    auto &gr = rounds[g][r];
    const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
    std::vector<std::string> names(n0.args.size());
    for (std::size_t a = 0; a < n0.args.size() && !gr.reduced; ++a) {
        if (wide_rd && a + 1u < n0.args.size() && a % 2u == 0u) {
            // (Operands a, a + 1 of the sum: adjacent slots of the node's operand array.)
            const auto w = wide_read(utname(gr.arg_tbl[a]));
            names[a] = w + ".x";
            names[a + 1u] = w + ".y";
            ++a;
            continue;
        }
        if (is_var(n0.args[a])) {
            names[a] = e.def(slabk(k, utname(gr.arg_tbl[a])));
        }
    }
    return names;
}

void cluster2_gen::emit_glue_compute(std::size_t g, std::uint32_t r, std::uint32_t k, const std::vector<std::string> &names)
{
    const auto &grp = pl.groups[g];
    auto &gr = rounds[g][r];
    const auto rep = grp.nodes[0];
    const auto &n0 = p.nodes[rep - n_eq];
    const auto saved = e.numpar_override;
    std::vector<std::pair<std::uint32_t, std::string>> saved_vals, saved_vals0;
    std::string fused_val;
    if (gr.reduced) {
        // Lane-reduced round (plan_lane_sums()): names[0] is the register of the first round which holds, on the five
        // adjacent lanes of a segment, the terms t0 .. t4 of a sum. Three row_shr steps leave ((t0 + t1) + (t2 + t3)) + t4,
        // the pairwise tree of the sum rule (additions commute: bit for bit), on the LAST lane of every segment:
        //   a = t + shr1(t)   lane 1: t1 + t0, lane 3: t3 + t2
        //   b = a + shr2(a)   lane 3: (t3 + t2) + (t1 + t0)
        //   c = t + shr1(b)   lane 4: t4 + b3
        // The other lanes end with partial sums, mixtures across segments or (row starts) whatever an out-of-row fetch
        // yields - zeros on the hardware (hy_dpp sets bound_ctrl), the lanes wrapped around the row under the emulator of
        // tests/emu -: none of it reaches a result (their stores: emit_step_body(), the norms: publish_sv()).
        const auto &t = names.at(0);
        const auto sa = e.def(t + " + hy_dpp<0x111>(" + t + ")");
        const auto sb = e.def(sa + " + hy_dpp<0x112>(" + sa + ")");
        fused_val = e.def(t + " + hy_dpp<0x111>(" + sb + ")");
    } else if (!gr.coef_tbl.empty()) {
        // Sum of scaled products, pairwise like the sum rule: ((t0 + t1) + (t2 + t3)) + ..., t_i = c_i * p_i, the
        // first product of every pair fused into the addition.
        std::vector<std::string> terms;
        for (std::size_t a = 0; a + 1u < names.size(); a += 2u) {
            const auto m = e.def(ssa_emitter::mul(coefname(gr.coef_tbl[a + 1u]), names[a + 1u]));
            terms.push_back(e.def("__builtin_fma(" + coefname(gr.coef_tbl[a]) + ", " + names[a] + ", " + m + ")"));
        }
        const bool odd = names.size() % 2u == 1u;
        while (terms.size() > 1u) {
            std::vector<std::string> nt;
            for (std::size_t i = 0; i + 1u < terms.size(); i += 2u) {
                nt.push_back(e.def(terms[i] + " + " + terms[i + 1u]));
            }
            if (terms.size() % 2u == 1u) {
                nt.push_back(terms.back());
            }
            terms = std::move(nt);
        }
        if (odd) {
            const auto a = names.size() - 1u;
            fused_val = terms.empty() ? e.def(ssa_emitter::mul(coefname(gr.coef_tbl[a]), names[a]))
                                      : e.def("__builtin_fma(" + coefname(gr.coef_tbl[a]) + ", " + names[a] + ", " + terms[0] + ")");
        } else {
            fused_val = terms[0];
        }
    }
    for (std::size_t a = 0; fused_val.empty() && a < n0.args.size(); ++a) {
        const auto &o = n0.args[a];
        if (is_var(o)) {
            saved_vals.emplace_back(o.idx, e.val(o.idx, k));
            e.val(o.idx, k) = names[a];
            // Constant operand: the linear rule of ssa_emitter::node() uses the value read at order 0.
            if (cu[o.idx] != 0) {
                if (k == 0u) {
                    gr.c0name.resize(n0.args.size());
                    gr.c0name[a] = names[a];
                } else {
                    saved_vals0.emplace_back(o.idx, e.val(o.idx, 0));
                    e.val(o.idx, 0) = gr.c0name.at(a);
                }
            }
        } else if (o.type == operand::kind::num) {
            e.numpar_override[&o] = dtname(gr.arg_tbl[a]);
        } else if (a < gr.par_name.size() && !gr.par_name[a].empty()) {
            e.numpar_override[&o] = gr.par_name[a];
        }
    }
    if (n0.kind == func_kind::prod && n0.args[0].type == operand::kind::num && n0.args[0].value == -1.) {
        e.numpar_override.erase(&n0.args[0]);
    }
    if (fused_val.empty()) {
        e.node(rep - n_eq, k);
    }
    const auto gval = fused_val.empty() ? e.val(rep, k) : fused_val;
    // NOTE: constant nodes are exported at every order too (zeros beyond order 0): a reader whose template position
    // pairs the constant with a variable in another cluster reads it at every order.
    if (gr.exported) {
        os << slabk(k, utname(gr.out_tbl)) << " = " << gval << ";\n";
    }
    for (auto it = saved_vals.rbegin(); it != saved_vals.rend(); ++it) {
        e.val(it->first, k) = it->second;
    }
    for (auto it = saved_vals0.rbegin(); it != saved_vals0.rend(); ++it) {
        e.val(it->first, 0) = it->second;
    }
    e.numpar_override = saved;

    // Fused state-variable recursion: x^[k+1] = src^[k] / (k + 1). In the merged schedule the a-th variable of
    // the chain runs a orders ahead (x^[k+1+a] from the coefficient of order k + a of its predecessor, which
    // the same lane has just produced): a position is then known one exchange earlier than the acceleration
    // of the same order, which is what lets cluster(k+1) and glue(k) share one round.
    for (std::size_t a = 0; a < gr.owners.size(); ++a) {
        const auto ord = k + 1u + (merged ? static_cast<std::uint32_t>(a) : 0u);
        if (ord > order) {
            continue;
        }
        const auto src = (a == 0u) ? gval : gr.owners[a - 1u].xname[ord - 1u];
        const auto x = e.div_const(src, ord);
        publish_sv(gr.owners[a], ord, x);
    }
}

// ---- Lane-pair cluster program ----
// Coefficient histories of a lane (SSA names by order), role A | role B:
//   aS: d_0 | d_2          aP: d_1 | b = sum of squares          aR: sa = (scaled) pow, both lanes
//   aRp: d_1 (a copy) | -(alpha + 1) j sa_j
// Convolution chains of order k (same FMA stream on both lanes), history part = indices 1 .. k-1:
//   c1 = sum aP[k-j] aR[j]   (A: d_1 * sa,  B: S1 = sum b[k-j] sa[j] of the pow recurrence)
//   c2 = sum aP[k-j] aRp[j]  (A: the order-k coefficient of d_1^2, B: S2 = sum b[k-j] j sa[j])
//   c3 = sum aS[k-j] aR[j]   (d_0 * sa | d_2 * sa)
//   c4 = sum_{j <= jmax} aS[k-j] aS[j] (+ the middle square): d_0^2 | d_2^2
// The pow recurrence (src/math/pow.cpp:517-549) k b_0 a_k = sum_{j<k} (k alpha - j (alpha + 1)) b_{k-j} a_j is linear
// in a: it is run directly on sa = c a, as alpha k S1 - (alpha + 1) S2.
// Per order the two lanes exchange (DPP quad_perm [1,0,3,2], no LDS): the partial sums of squares, then sa_k.
std::vector<std::string> cluster2_gen::emit_pair_reads(std::uint32_t k)
{
    const auto rd = [&](std::size_t t) { return e.def(slabk(k, utname(t))); };
    return std::vector<std::string>{rd(pt.s0), rd(pt.s1), rd(pt.p0), rd(pt.p1)};
}

void cluster2_gen::emit_pair_compute(std::uint32_t k, const std::vector<std::string> &rdv)
{
    const auto &es0 = rdv[0], &es1 = rdv[1], &ep0 = rdv[2], &ep1 = rdv[3];
    aS[k] = e.def(es0 + " - " + es1);
    const auto dP = e.def(ep0 + " - " + ep1);
    std::string sqS, sqy;
    if (k == 0u) {
        sqS = e.def(ssa_emitter::mul(aS[0], aS[0]));
        sqy = e.def(ssa_emitter::mul(dP, dP));
    } else {
        const auto acc4 = e.chain(hc4, aS[k], aS[0]);
        sqS = (k % 2u == 0u) ? e.def("__builtin_fma(2.0, " + acc4 + ", " + hmid + ")") : e.def(acc4 + " + " + acc4);
        // (A: 2 d_1[k] d_1[0] on top of the symmetric history sum; ap0x2 = 2 aP[0].)
        sqy = e.chain(hc2, dP, ap0x2);
    }
    // NOTE: role-dependent values are formed arithmetically with the lane constants fA / fB (1.0 on the lanes of
    // the role, 0.0 on the others) instead of selects (two v_cndmask per double): lane B reads the same slot twice
    // for the second difference, so that its dP is an exact zero.
    const auto mine = e.def("__builtin_fma(fA, " + sqy + ", " + sqS + ")");
    const auto oth = e.def("hy_swap1(" + mine + ")");
    const auto r2 = e.def(mine + " + " + oth);
    aP[k] = e.def("__builtin_fma(" + std::string((pow_norm && k >= 1u) ? "rb1n" : "fB") + ", " + r2 + ", " + dP + ")");
    std::string c1a;
    if (k == 0u) {
        // NOTE: the sum of squares is the same on both lanes: each of them evaluates the pow itself.
        const auto a0 = e.pow_eval(r2, pp.ex);
        aR[0] = pp.sc >= 0 ? e.def(ssa_emitter::mul(dtname(pt.csc), a0)) : a0;
        // (Zero on lane A: its quotient below is then an exact zero and sa_k = own + partner's.)
        rb1 = e.def("isB ? (1.0 / " + aP[0] + ") : 0.0");
        if (pow_norm) {
            os << "const double rb1n = " << rb1 << ";\n";
        }
        ap0x2 = e.def(aP[0] + " + " + aP[0]);
    } else {
        c1a = e.chain(hc1, aP[k], aR[0]);
        // NOTE: lane B keeps -(alpha + 1) j sa_j in aRp, so that its c2 chain is -(alpha + 1) S2 right away.
        std::string num;
        if (pow_norm) {
            const auto m = e.def(ssa_emitter::mul(fp_literal(pp.ex), c1a));
            const auto sab = hc2.empty() ? m
                                         : e.def("__builtin_fma(" + hc2 + ", " + fp_literal(1. / static_cast<double>(k)) + ", " + m + ")");
            // (Masked to the B lanes: the value doubles as the operand of aRp below.)
            const auto t = e.def(ssa_emitter::mul("fB", sab));
            aR[k] = e.def("hy_dpp<0xF5>(" + t + ")");
            if (k + 2u <= order) {
                aRp[k] = e.def("__builtin_fma(" + fp_literal(-(pp.ex + 1.) * static_cast<double>(k)) + ", " + t + ", " + dP + ")");
            }
        } else {
        if (hc2.empty()) {
            num = e.def(ssa_emitter::mul(fp_literal(pp.ex * static_cast<double>(k)), c1a));
        } else {
            num = e.def(fp_literal(pp.ex * static_cast<double>(k)) + " * " + c1a + " + " + hc2);
        }
        // Division by k * b_0 (src/math/pow.cpp:546-549) without a division sequence on the critical path:
        // n = num * RN(1 / k), q0 = n * r with r = RN(1 / b_0); residual rem = n - b_0 * q0 (exact, FMA);
        // q = q0 + rem * r (Markstein: the correctly-rounded n / b_0 unless r is off by more than an ulp in a
        // halfway case; n itself carries the rounding of the scaling by 1 / k, so q is within 1.5 ulp of the
        // quotient num / (k b_0) the reference rounds once).
        const auto nk = (k == 1u) ? num : e.def(ssa_emitter::mul(num, fp_literal(1. / static_cast<double>(k))));
        const auto q0 = e.def(ssa_emitter::mul(nk, rb1));
        const auto rem = e.def("__builtin_fma(-" + aP[0] + ", " + q0 + ", " + nk + ")");
        const auto sab = e.def("__builtin_fma(" + rem + ", " + rb1 + ", " + q0 + ")");
        const auto sao = e.def("hy_swap1(" + sab + ")");
        aR[k] = e.def(sab + " + " + sao);
        }
    }
    if (!pow_norm && k >= 1u && k + 2u <= order) {
        const auto t = e.def(ssa_emitter::mul("fB", aR[k]));
        aRp[k] = e.def("__builtin_fma(" + fp_literal(-(pp.ex + 1.) * static_cast<double>(k)) + ", " + t + ", " + dP + ")");
    }
    std::string prS, prP;
    if (k == 0u) {
        prS = e.def(ssa_emitter::mul(aS[0], aR[0]));
        prP = e.def(ssa_emitter::mul(aP[0], aR[0]));
    } else {
        prS = e.chain(e.chain(hc3, aS[k], aR[0]), aS[0], aR[k]);
        prP = e.chain(c1a, aP[0], aR[k]);
    }
    os << slabk(k, utname(pt.os)) << " = " << prS << ";\n";
    os << slabk(k, utname(pt.op)) << " = " << prP << ";\n";
    if (has_rx && !fuse_rx) {
        const auto rS = e.def(ssa_emitter::mul(dtname(pt.crs), prS));
        const auto rP = e.def(ssa_emitter::mul(dtname(pt.crp), prP));
        os << slabk(k, utname(pt.rs)) << " = " << rS << ";\n";
        os << slabk(k, utname(pt.rp)) << " = " << rP << ";\n";
    }
    // History parts of order K = k + 1 (indices 1 .. k), the four chains interleaved term by term.
    hc1.clear();
    hc2.clear();
    hc3.clear();
    hc4.clear();
    hmid.clear();
    const auto K = k + 1u;
    if (K < order && K >= 2u) {
        const auto jmax = (K % 2u == 1u) ? (K - 1u) / 2u : (K - 2u) / 2u;
        for (std::uint32_t j = 1; j < K; ++j) {
            hc1 = e.chain(hc1, aP[K - j], aR[j]);
            hc2 = e.chain(hc2, aP[K - j], aRp[j]);
            hc3 = e.chain(hc3, aS[K - j], aR[j]);
            if (j <= jmax) {
                hc4 = e.chain(hc4, aS[K - j], aS[j]);
            }
        }
        if (K % 2u == 0u) {
            hmid = e.def(ssa_emitter::mul(aS[K / 2u], aS[K / 2u]));
        }
    }
}

// ---- One-lane pair program ("v5") ----
// Histories of a lane (SSA names by order): sD[i] = d_i (i = 0, 1, 2), sB = b_k / b_0 (k >= 1; b = sum of squares),
// sA = sa = (scaled) pow. Chains of order k, history part = indices 1 .. k-1:
//   q_i = sum_{j <= jmax} d_i[k-j] d_i[j]                      (half of the symmetric sum of d_i^2, see below)
//   T   = sum_j sB[k-j] sA[j]                                  (S1 of the pow recurrence)
//   U   = sum of the suffix sums of T's terms = sum_j j sB[k-j] sA[j]   (S2; terms taken in the order j = k-1 .. 1)
//   c_i = sum_j d_i[k-j] sA[j]                                 (d_i * sa)
// b_k = 2 (q_0 + q_1 + q_2) (+ the middle squares at even orders): the factor 2 is exact, so the HALF sum
// bh = (q_0 + 0.5 mid_0) + ... is formed instead and the doubling is folded into the normalisation constant
// rb2 = 2 RN(1 / b_0). a_k = alpha (T + sB[k] a_0) - ((alpha + 1) / k) U (src/math/pow.cpp:517-549 divided by k b_0).
std::vector<std::string> cluster2_gen::emit_single_reads(std::uint32_t k)
{
    std::vector<std::string> r(6);
    if (vexch) {
        // The velocity coefficients of order k - 1 of the two bodies (row k - 1 of the jets; order 0: their current
        // positions, behind the rows).
        const auto row = k == 0u ? jet_rows_doubles : static_cast<std::uint64_t>(k - 1u) * spw * n_colp;
        for (std::uint32_t i = 0; i < 3u; ++i) {
            for (std::uint32_t sd = 0; sd < 2u; ++sd) {
                r[2u * i + sd] = e.def("jetq[" + utname(st1.s[i][sd]) + " + " + std::to_string(row) + "u]");
            }
        }
        return r;
    }
    if (wide_rd) {
        // (x, y) of the two bodies with one ds_read_b128 each, then the two z.
        for (std::uint32_t sd = 0; sd < 2u; ++sd) {
            const auto w = wide_read(utname(st1.s[0][sd]));
            r[0u + sd] = w + ".x";
            r[2u + sd] = w + ".y";
        }
        for (std::uint32_t sd = 0; sd < 2u; ++sd) {
            r[4u + sd] = e.def(slabk(k, utname(st1.s[2][sd])));
        }
        return r;
    }
    for (std::uint32_t i = 0; i < 3u; ++i) {
        r[2u * i] = e.def(slabk(k, utname(st1.s[i][0])));
        r[2u * i + 1u] = e.def(slabk(k, utname(st1.s[i][1])));
    }
    return r;
}

void cluster2_gen::emit_single_compute(std::uint32_t k, const std::vector<std::string> &rdv)
{
    for (std::uint32_t i = 0; i < 3u; ++i) {
        sD[i][k] = e.def(rdv[2u * i] + " - " + rdv[2u * i + 1u]);
        if (vexch && k >= 2u) {
            // (d^[k] = (v_a^[k-1] - v_b^[k-1]) RN(1 / k).)
            sD[i][k] = e.def(ssa_emitter::mul(sD[i][k], fp_literal(1. / static_cast<double>(k))));
        }
    }
    std::string pr[3];
    if (k == 0u) {
        // (Products rounded one by one, summed pairwise like the reference's sum_sq: src/detail/sum_sq.cpp:120-245.)
        std::string sq[3];
        for (std::uint32_t i = 0; i < 3u; ++i) {
            sq[i] = e.def(ssa_emitter::mul(sD[i][0], sD[i][0]));
        }
        const auto s01 = e.def(sq[0] + " + " + sq[1]);
        const auto r2 = e.def(s01 + " + " + sq[2]);
        sB[0] = r2;
        const auto a0 = e.pow_eval(r2, pp.ex);
        sA[0] = pp.sc >= 0 ? e.def(ssa_emitter::mul(dtname(st1.csc), a0)) : a0;
        const auto rb = e.def("1.0 / " + r2);
        os << "const double rb2 = " << rb << " + " << rb << ";\n";
        os << "const double arbA = " << fp_literal(pp.ex) << " * (rb2 * " << sA[0] << ");\n";
        for (std::uint32_t i = 0; i < 3u; ++i) {
            pr[i] = e.def(ssa_emitter::mul(sD[i][0], sA[0]));
        }
    } else {
        // The dependent chain from the exchange to the stores decides how soon the next round can start, so
        // everything which does not need an order-k input was folded into the history accumulators at the end of the
        // previous round (the middle squares into hq, alpha T - ((alpha + 1) / k) U into pow_pre): what is left is
        // sub -> fma -> add -> add -> fma (sa_k) -> fma (products) -> mul (reactions).
        std::string bh;
        if (merged_sq) {
            bh = hq[0];
            for (std::uint32_t i = 0; i < 3u; ++i) {
                bh = e.chain(bh, sD[i][k], sD[i][0]);
            }
        } else {
            std::string q[3];
            for (std::uint32_t i = 0; i < 3u; ++i) {
                q[i] = e.chain(hq[i], sD[i][k], sD[i][0]);
            }
            const auto q01 = e.def(q[0] + " + " + q[1]);
            bh = e.def(q01 + " + " + q[2]);
        }
        // sa_k = alpha (T + (b_k / b_0) sa_0) - ((alpha + 1) / k) U with b_k / b_0 = rb2 bh: alpha rb2 sa_0 is a constant
        // of the step (arbA).
        sA[k] = pow_pre.empty() ? e.def(ssa_emitter::mul(bh, "arbA")) : e.def("__builtin_fma(" + bh + ", arbA, " + pow_pre + ")");
        sB[k] = e.def(ssa_emitter::mul("rb2", bh));
        for (std::uint32_t i = 0; i < 3u; ++i) {
            pr[i] = e.chain(e.chain(hcx[i], sD[i][k], sA[0]), sD[i][0], sA[k]);
        }
    }
    for (std::uint32_t i = 0; i < 3u; ++i) {
        emit_store(slabk(k, utname(st1.o[i])) + " = " + pr[i] + ";\n");
    }
    for (std::uint32_t i = 0; pp.rx[0] >= 0 && !fuse_rx && i < 3u && !exp_norx; ++i) {
        // (The reaction on the second body of the pair: c * (d_i * sa), src/model/nbody.cpp:113-130.)
        const auto rxv = e.def(ssa_emitter::mul("crs_r", pr[i]));
        emit_store(slabk(k, utname(st1.r[i])) + " = " + rxv + ";\n");
    }
    if (any_pad && k >= 1u) {
        for (unsigned i = 0; i < pad_dep; ++i) {
            os << "asm volatile(\"v_fma_f64 %0, %0, %0, %0\" : \"+v\"(hy_pad0));\n";
        }
        for (unsigned i = 0; i < pad_regs; ++i) {
            os << "asm volatile(\"v_fma_f64 %0, %1, %0, %0\" : \"+v\"(hy_pad0) : \"v\"(hy_rp" << i << "));\n";
        }
        // (Written-out LDS stores of the first product to its own slot once more: same value, same address. The
        // compiler's lgkmcnt bookkeeping stays conservative: LDS operations complete in order.)
        for (unsigned i = 0; i < pad_st % 100u; ++i) {
            os << "asm volatile(\"ds_write_b64 %0, %1\" ::\"v\"((unsigned)(unsigned long long)&" << slabk(k, utname(st1.o[0]))
               << "), \"v\"(" << pr[0] << ") : \"memory\");\n";
        }
        // (pad_st >= 100: 16-byte stores - the first product and its neighbour in the array written back as a pair.)
        for (unsigned i = 0; i < pad_st / 100u; ++i) {
            os << "{\nhy_d2 hy_pv;\nhy_pv.x = " << pr[0] << ";\nhy_pv.y = " << pr[0] << ";\n"
               << "asm volatile(\"ds_write_b128 %0, %1\" ::\"v\"((unsigned)(unsigned long long)(slab + (" << dummy_base
               << "u & ~1u))), \"v\"(hy_pv) : \"memory\");\n}\n";
        }
        // (LDS reads of the velocity coefficients of the previous order once more, summed into a dummy: the reads of
        // this round cannot be shared with them - the wave barrier between the rounds is a memory clobber.)
        for (unsigned i = 0; vexch && k >= 2u && i < pad_ld && i < 6u; ++i) {
            os << "hy_pad4 = hy_pad4 + jetq[" << utname(st1.s[i % 3u][i / 3u]) << " + "
               << static_cast<std::uint64_t>(k - 2u) * spw * n_colp << "u];\n";
        }
        for (unsigned i = 0; i < pad_salu; ++i) {
            os << "asm volatile(\"s_nop 0\");\n";
        }
    }
    if (prio_switch) {
        // (End of the latency-critical part of the round: the chains below are bulk work.)
        os << "__builtin_amdgcn_s_setprio(0);\n";
    }
    if (any_pad && k >= 1u) {
        for (unsigned i = 0; i < pad_chain; ++i) {
            os << "asm volatile(\"v_fma_f64 %0, %0, %0, %0\" : \"+v\"(hy_pad" << (1u + i % 4u) << "));\n";
        }
    }
}

void cluster2_gen::emit_single_history(std::uint32_t k)
{
    // History parts of order K = k + 1 (terms without an order-K operand) and the T / U chains of the pow recurrence,
    // whose first term is the newest one.
    for (std::uint32_t i = 0; i < 3u; ++i) {
        hq[i].clear();
        hm[i].clear();
        hcx[i].clear();
    }
    hT.clear();
    hU.clear();
    const auto K = k + 1u;
    if (K < order && K >= 2u) {
        const auto jmax = (K % 2u == 1u) ? (K - 1u) / 2u : (K - 2u) / 2u;
        for (std::uint32_t j = 1; j < K; ++j) {
            // (T / U take their terms in the order j = K-1 .. 1: the first term enters U K-1 times, the last one once.)
            const auto jd = K - j;
            hT = e.chain(hT, sB[K - jd], sA[jd]);
            hU = hU.empty() ? hT : e.def(hU + " + " + hT);
            for (std::uint32_t i = 0; i < 3u; ++i) {
                hcx[i] = e.chain(hcx[i], sD[i][K - j], sA[j]);
                if (j <= jmax) {
                    auto &acc = hq[merged_sq ? 0u : i];
                    acc = e.chain(acc, sD[i][K - j], sD[i][j]);
                }
            }
        }
        if (K % 2u == 0u) {
            for (std::uint32_t i = 0; i < 3u; ++i) {
                if (merged_sq) {
                    // (One running sum of the three middle squares.)
                    hm[0] = e.chain(i == 0u ? std::string{} : hm[0], sD[i][K / 2u], sD[i][K / 2u]);
                } else {
                    hm[i] = e.def(ssa_emitter::mul(sD[i][K / 2u], sD[i][K / 2u]));
                }
            }
        }
        // Off the critical path of round K: the middle squares join the half sums, the two sums of the pow
        // recurrence are combined.
        if (K % 2u == 0u) {
            for (std::uint32_t i = 0; i < (merged_sq ? 1u : 3u); ++i) {
                hq[i] = hq[i].empty() ? e.def(ssa_emitter::mul("0.5", hm[i]))
                                      : e.def("__builtin_fma(0.5, " + hm[i] + ", " + hq[i] + ")");
            }
        }
        const auto t1 = e.def(ssa_emitter::mul(fp_literal(-(pp.ex + 1.) / static_cast<double>(K)), hU));
        pow_pre = e.def("__builtin_fma(" + fp_literal(pp.ex) + ", " + hT + ", " + t1 + ")");
    } else {
        pow_pre.clear();
    }
}

// Order k of the cluster phase: the lane-pair program, or the template cluster of the pipelined kernel.
void cluster2_gen::emit_cluster(std::uint32_t k)
{
    if (pair_split) {
        emit_pair_order(k);
        return;
    }
    for (std::uint32_t part = 1; part < n_parts; ++part) {
        e.emit_partials(t0_ids, k, part, n_parts);
    }
    for (std::uint32_t x = 0; x < n_ext; ++x) {
        if (ext_const[x] != 0 && k > 0u) {
            // A constant input of every cluster (e.g. -par[i]): read once, at order 0.
            e.val(pl.ext_u[0][x], k) = "0.0";
            continue;
        }
        e.val(pl.ext_u[0][x], k) = e.def(slabk(k, utname(ext_tbl[x])));
    }
    if (overlap) {
        sched_fence();
        e.emit_partials_sel(t0_ids, k + 1u, psel::early_b);
        if (fence2) {
            sched_fence();
        }
    }
    for (const auto u : t0()) {
        e.node_finish(u - n_eq, k);
    }
    for (std::uint32_t x = 0; x < n_out; ++x) {
        os << slabk(k, utname(out_tbl[x])) << " = " << e.val(t0()[pl.out_pos[x]], k) << ";\n";
    }
}

// (which = 0: every field; 1: the fields a step changes; 2: the others - final time and limits, which only change when a
// system is picked up: an LDS store is the most expensive instruction of the kernel.)
// (3: the fields a plain step changes - plain_step: neither the flags nor anything a clamped or finished step sets.)
void cluster2_gen::bk_store(int which)
{
    std::uint32_t f = 0;
    for (const auto *nm : bk_fields_d) {
        const std::string n_ = bk_field(nm);
        const bool constant = n_ == "tfin.hi" || n_ == "tfin.lo" || n_ == "mdt" || n_ == "step_lim" || n_ == "thr";
        if (!n_.empty() && (which == 0 || ((which == 1 || which == 3) != constant))) {
            src << "bk[" << f << "] = " << n_ << ";\n";
        }
        ++f;
    }
    if (which == 2) {
        return;
    }
    src << "bk[" << f++ << "] = __longlong_as_double((long long)n_steps);\n";
    src << "bk[" << f++ << "] = __longlong_as_double((long long)iter);\n";
    src << "bk[" << f++ << "] = __longlong_as_double((long long)outcome);\n";
    if (which == 3) {
        return;
    }
    src << "bk[" << f++ << "] = __longlong_as_double((long long)((t_dir ? 1 : 0) | (nf_seen != 0 ? 2 : 0) | (gfin ? 4 : 0)));\n";
}

// (The field of the parked record under this name: with plain steps the remaining time is not carried - the lower bound of
// its magnitude sits in the word of its high part and the word of its low part is free, "".)
std::string cluster2_gen::bk_field(const char *nm) const
{
    const std::string n_ = nm;
    if (plain_step && n_ == "rem.hi") {
        return "rlb";
    }
    return (plain_step && n_ == "rem.lo") ? std::string{} : n_;
}

void cluster2_gen::bk_load()
{
    std::uint32_t f = 0;
    for (const auto *nm : bk_fields_d) {
        if (const auto n_ = bk_field(nm); !n_.empty()) {
            src << n_ << " = bk[" << f << "];\n";
        }
        ++f;
    }
    src << "n_steps = (u64)__double_as_longlong(bk[" << f++ << "]);\n";
    src << "iter = (u64)__double_as_longlong(bk[" << f++ << "]);\n";
    src << "outcome = (i64)__double_as_longlong(bk[" << f++ << "]);\n";
    src << "{\nconst long long fl = __double_as_longlong(bk[" << f++ << "]);\nt_dir = (fl & 1) != 0;\nnf_seen = (fl & 2) != 0 ? 1 : 0;\ngfin = (fl & 4) != 0;\n}\n";
}

// (A value the final evaluation reads: the name it was given above, or the read itself.)
std::string cluster2_gen::tail_val(const std::vector<std::string> &names, std::uint32_t k, const std::string &ex)
{
    if (names.empty()) {
        return ex;
    }
    ++n_trd_used;
    return names.at(k);
}

} // namespace heyoka_amd::cluster2_detail
