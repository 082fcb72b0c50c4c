// "Cluster" code generation mode: one ODE system per group of L lanes, jets resident in registers.
//
// The Taylor recursion of a nonlinear node (product, sum of squares, pow, sin/cos, ...) at order k
// reads *all* lower orders of its operands: for an N-body system that history (15 pairs x 6 jets x
// 20 orders for the outer Solar System) cannot live in the registers of a single lane, and parking
// it in HBM makes the step bandwidth-bound at a small fraction of the FP64 rate. This generator
// instead partitions the decomposition (reference: taylor_dc_t, src/taylor_01.cpp:848-1008) into
//
//   * clusters - connected components under "history" edges (a nonlinear node and the operands whose
//     full history it needs). All clusters must be isomorphic (one code path, SIMT-friendly); each
//     cluster is owned by one lane of the system's lane group and keeps its jets in that lane's VGPRs;
//   * glue - linear nodes (sums, differences, products by constants) and the state-variable
//     recursion x^[k] = rhs^[k-1] / k, which only ever need *current-order* values. These are
//     exchanged between the lanes of a group through a per-system LDS slab holding the order-k
//     coefficient of every exported u variable, and are evaluated in SIMT "rounds" driven by small
//     per-lane slot tables.
//
// Per-order flow: state-variable recursion -> clusters -> glue levels, separated by wave-level LDS
// synchronisations (a system never spans wavefronts, hence no s_barrier). The state-variable jets go to
// a small per-wave scratch (L2 / Infinity-Cache resident, laid out [order][system][variable] so that
// a wave's accesses are contiguous), are reduced for the step-size selector with wavefront shuffles,
// and are read back for the Horner / compensated update. Blocks are persistent and pull groups of
// systems from a device-side work queue, so that the scratch is proportional to the number of
// resident waves rather than to the number of systems.
//
// The arithmetic of every node is emitted by the same ssa_emitter as the unrolled mode (reference
// formulas cited in hip_emit_detail.hpp).
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <limits>
#include <map>
#include <numeric>
#include <set>

#include "hip_emit_cluster_plan.hpp"
#include "hip_emit_detail.hpp"

namespace heyoka_amd
{

namespace
{

using emit_detail::ssa_emitter;

using cluster_detail::cluster_plan;
using cluster_detail::glue_group;
using cluster_detail::is_var;

} // namespace

// Version 1 of the cluster kernel: separate state-variable phase, 4 LDS synchronisations per order.
// Returns a module with an empty source (and the reason in why_not) if cluster mode is not applicable.
emitted_module emit_cluster_v1(const taylor_program &p, const emit_options &opts, emit_refusal &why_not, bool multi_class)
{
    using emit_detail::prelude;
    using emit_detail::rhofac;
    using cluster_detail::cluster_class;

    emitted_module ret;
    cluster_plan pl;
    cluster_detail::plan_limits lim;
    lim.multi_class = multi_class;
    why_not = cluster_detail::make_plan(p, opts.order, pl, lim);
    if (!why_not.empty()) {
        return ret;
    }

    const auto n_eq = p.n_eq, order = opts.order, L = pl.L, spw = pl.spw;
    const std::uint32_t bs = 256, wpb = bs / 64u;
    const auto nc = static_cast<std::uint32_t>(pl.clusters.size());
    // The classes of clusters: one section of code each (a single-class plan is the class of all the clusters).
    std::vector<cluster_class> classes = pl.classes;
    if (classes.empty()) {
        cluster_class c;
        c.members.resize(nc);
        std::iota(c.members.begin(), c.members.end(), 0u);
        c.level = pl.cluster_level;
        c.cst_pos = pl.cst_pos;
        c.cst_val = pl.cst_val;
        c.out_pos = pl.out_pos;
        c.stored_pos = pl.stored_pos;
        classes.push_back(std::move(c));
    }
    const auto sv_rounds = (n_eq + L - 1u) / L;
    const auto n_col = sv_rounds * L;

    // Dummy slots for idle lanes (they replicate real work and write to slots nobody reads).
    std::uint32_t max_round_outputs = 1u;
    for (const auto &cls : classes) {
        max_round_outputs = std::max<std::uint32_t>(max_round_outputs, static_cast<std::uint32_t>(cls.out_pos.size()));
    }
    const auto dummy_base = pl.n_slots;
    const auto n_slots_tot = pl.n_slots + max_round_outputs;
    // Pad the per-system slab to an odd number of doubles (bank spreading between the systems of a wave).
    const auto slab_stride = n_slots_tot | 1u;

    // ---- per-lane tables (unsigned short slots, double constants) ----
    std::vector<std::vector<std::uint32_t>> utbl; // each entry: L values
    std::vector<std::vector<double>> dtbl;
    const auto add_utbl = [&](std::vector<std::uint32_t> v) {
        utbl.push_back(std::move(v));
        return utbl.size() - 1u;
    };
    const auto add_dtbl = [&](std::vector<double> v) {
        dtbl.push_back(std::move(v));
        return dtbl.size() - 1u;
    };

    ssa_emitter e(p, order);
    auto &os = e.os;
    // The body is emitted into a separate stream first, because the tables it needs are only known
    // once the whole body has been generated.
    std::ostringstream body;

    // Cluster tables, per class: lane l of a system holds cluster l of the class (idle lanes replicate its first one).
    struct class_tbls {
        std::vector<std::size_t> ext_tbl, out_tbl, cst_tbl;
    };
    std::vector<class_tbls> ctb(classes.size());
    std::vector<std::pair<std::string, std::size_t>> cst_names; // (name of the per-lane constant, its double table)
    for (std::size_t ci = 0; ci < classes.size(); ++ci) {
        const auto &cls = classes[ci];
        const auto ncl = static_cast<std::uint32_t>(cls.members.size());
        const auto c0 = cls.members[0];
        const auto &t0 = pl.clusters[c0];
        const auto n_ext = static_cast<std::uint32_t>(pl.ext_u[c0].size());
        const auto cluster_at = [&](std::uint32_t l) { return cls.members[l < ncl ? l : 0u]; };
        for (std::uint32_t x = 0; x < n_ext; ++x) {
            std::vector<std::uint32_t> v(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                v[l] = static_cast<std::uint32_t>(pl.slot_of[pl.ext_u[cluster_at(l)][x]]);
            }
            ctb[ci].ext_tbl.push_back(add_utbl(std::move(v)));
        }
        for (std::uint32_t x = 0; x < cls.out_pos.size(); ++x) {
            std::vector<std::uint32_t> v(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                v[l] = l < ncl ? static_cast<std::uint32_t>(pl.slot_of[pl.clusters[cls.members[l]][cls.out_pos[x]]]) : dummy_base + x;
            }
            ctb[ci].out_tbl.push_back(add_utbl(std::move(v)));
        }
        for (std::uint32_t x = 0; x < cls.cst_pos.size(); ++x) {
            std::vector<double> v(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                v[l] = cls.cst_val[l < ncl ? l : 0u][x];
            }
            ctb[ci].cst_tbl.push_back(add_dtbl(std::move(v)));
            const auto [q, a] = cls.cst_pos[x];
            const auto nm = "ccst" + std::to_string(ci) + "_" + std::to_string(x);
            e.numpar_override[&p.nodes[t0[q] - n_eq].args[a]] = nm;
            cst_names.emplace_back(nm, ctb[ci].cst_tbl.back());
        }
    }

    // State-variable rounds: variable index of lane l in round r is r * L + l (clamped for padding lanes).
    struct sv_round {
        std::size_t in_tbl = 0, out_tbl = 0, cst_tbl = 0;
        bool all_var = true, any_var = false;
    };
    std::vector<sv_round> svr(sv_rounds);
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        std::vector<std::uint32_t> vin(L), vout(L);
        std::vector<double> vc(L, 0.);
        for (std::uint32_t l = 0; l < L; ++l) {
            const auto i = r * L + l;
            const auto ii = i < n_eq ? i : r * L; // padding lanes replicate the first variable of the round
            const auto &d = p.sv_defs[ii];
            if (d.type == operand::kind::uvar) {
                vin[l] = static_cast<std::uint32_t>(pl.slot_of[d.idx]);
                svr[r].any_var = true;
            } else {
                vin[l] = 0;
                svr[r].all_var = false;
                if (d.type == operand::kind::par) {
                    return ret.notes = "param", why_not = "state variable defined by a runtime parameter", ret;
                }
                vc[l] = d.value;
            }
            vout[l] = i < n_eq ? static_cast<std::uint32_t>(pl.slot_of[i]) : dummy_base;
        }
        if (svr[r].any_var && !svr[r].all_var) {
            why_not = "mixed constant / variable state-variable definitions in one round";
            return ret;
        }
        svr[r].in_tbl = add_utbl(std::move(vin));
        svr[r].out_tbl = add_utbl(std::move(vout));
        svr[r].cst_tbl = add_dtbl(std::move(vc));
    }

    // ---- emission helpers ----
    const auto sync = [&]() { os << "HY_WSYNC();\n"; };
    const auto utname = [](std::size_t t) { return "ut" + std::to_string(t); };
    const auto dtname = [](std::size_t t) { return "dt" + std::to_string(t); };

    // Glue group emission at order k: rounds over the nodes of the group.
    struct glue_round_tbls {
        std::vector<std::size_t> arg_tbl; // per arg: utbl (var) or dtbl (const) index
        std::size_t out_tbl = 0;
    };
    std::vector<std::vector<glue_round_tbls>> glue_tbls(pl.groups.size());
    for (std::size_t g = 0; g < pl.groups.size(); ++g) {
        const auto &grp = pl.groups[g];
        const auto n_nodes = static_cast<std::uint32_t>(grp.nodes.size());
        const auto rounds = (n_nodes + L - 1u) / L;
        const auto &n0 = p.nodes[grp.nodes[0] - n_eq];
        for (std::uint32_t r = 0; r < rounds; ++r) {
            glue_round_tbls rt;
            for (std::size_t a = 0; a < n0.args.size(); ++a) {
                if (is_var(n0.args[a])) {
                    std::vector<std::uint32_t> v(L);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        const auto j = r * L + l;
                        const auto u = grp.nodes[j < n_nodes ? j : r * L];
                        v[l] = static_cast<std::uint32_t>(pl.slot_of[p.nodes[u - n_eq].args[a].idx]);
                    }
                    rt.arg_tbl.push_back(add_utbl(std::move(v)));
                } else if (n0.args[a].type == operand::kind::num) {
                    std::vector<double> v(L);
                    for (std::uint32_t l = 0; l < L; ++l) {
                        const auto j = r * L + l;
                        const auto u = grp.nodes[j < n_nodes ? j : r * L];
                        v[l] = p.nodes[u - n_eq].args[a].value;
                    }
                    rt.arg_tbl.push_back(add_dtbl(std::move(v)));
                } else {
                    rt.arg_tbl.push_back(0);
                }
            }
            std::vector<std::uint32_t> v(L);
            for (std::uint32_t l = 0; l < L; ++l) {
                const auto j = r * L + l;
                v[l] = j < n_nodes ? static_cast<std::uint32_t>(pl.slot_of[grp.nodes[j]]) : dummy_base;
            }
            rt.out_tbl = add_utbl(std::move(v));
            glue_tbls[g].push_back(std::move(rt));
        }
    }

    // Emit one glue group at order k by temporarily aliasing the first node of each round: the node
    // rule is emitted once per round with operands read from the slab through the lane's tables.
    // Constant operands (constant_uvars()): the value a round has read at order 0 is the one the linear rule
    // c^[0] * x^[k] of ssa_emitter::node() uses at every order (same position in all the nodes of a group: the shape key
    // of a group does not distinguish them, so const-ness is checked over the whole group).
    std::map<std::tuple<std::size_t, std::size_t, std::size_t>, std::string> glue_c0;
    const auto emit_glue_group = [&](std::size_t g, std::uint32_t k) {
        const auto &grp = pl.groups[g];
        const auto rep = grp.nodes[0];
        const auto &n0 = p.nodes[rep - n_eq];
        for (std::size_t r = 0; r < glue_tbls[g].size(); ++r) {
            const auto &rt = glue_tbls[g][r];
            std::map<const operand *, std::string> saved = e.numpar_override;
            std::vector<std::pair<std::uint32_t, std::string>> saved_vals;
            std::vector<std::pair<std::uint32_t, std::string>> saved_vals0;
            for (std::size_t a = 0; a < n0.args.size(); ++a) {
                const auto &o = n0.args[a];
                if (is_var(o)) {
                    const auto nm = e.def("slab[" + utname(rt.arg_tbl[a]) + "]");
                    saved_vals.emplace_back(o.idx, e.val(o.idx, k));
                    e.val(o.idx, k) = nm;
                    if (e.cu[o.idx] != 0) {
                        if (k == 0u) {
                            glue_c0[{g, r, a}] = nm;
                        } else {
                            saved_vals0.emplace_back(o.idx, e.val(o.idx, 0));
                            e.val(o.idx, 0) = glue_c0.at({g, r, a});
                        }
                    }
                } else if (o.type == operand::kind::num) {
                    e.numpar_override[&o] = dtname(rt.arg_tbl[a]);
                }
            }
            // NOTE: structural numbers (-1 of a negation) keep their literal value; constants are
            // read from the per-lane table only at the orders where the rule uses them.
            if (n0.kind == func_kind::prod && n0.args[0].type == operand::kind::num && n0.args[0].value == -1.) {
                e.numpar_override.erase(&n0.args[0]);
            }
            e.node(rep - n_eq, k);
            os << "slab[" << utname(rt.out_tbl) << "] = " << e.val(rep, k) << ";\n";
            // Restore.
            for (auto it = saved_vals.rbegin(); it != saved_vals.rend(); ++it) {
                e.val(it->first, k) = it->second;
            }
            for (auto it = saved_vals0.rbegin(); it != saved_vals0.rend(); ++it) {
                e.val(it->first, 0) = it->second;
            }
            e.numpar_override = std::move(saved);
        }
    };

    // Code of class ci at order k (the template cluster of the class; the lanes differ by their slot tables / constants).
    const auto emit_cluster = [&](std::size_t ci, std::uint32_t k) {
        const auto &cls = classes[ci];
        const auto c0 = cls.members[0];
        const auto &t0 = pl.clusters[c0];
        for (std::size_t x = 0; x < ctb[ci].ext_tbl.size(); ++x) {
            e.val(pl.ext_u[c0][x], k) = e.def("slab[" + utname(ctb[ci].ext_tbl[x]) + "]");
        }
        for (const auto u : t0) {
            e.node(u - n_eq, k);
        }
        for (std::size_t x = 0; x < cls.out_pos.size(); ++x) {
            os << "slab[" << utname(ctb[ci].out_tbl[x]) << "] = " << e.val(t0[cls.out_pos[x]], k) << ";\n";
        }
    };

    // All the levels of order k (k < order).
    const auto emit_levels = [&](std::uint32_t k) {
        for (std::uint32_t lev = 1; lev <= pl.max_level; ++lev) {
            for (std::size_t ci = 0; ci < classes.size(); ++ci) {
                if (classes[ci].level == lev) {
                    emit_cluster(ci, k);
                }
            }
            for (std::size_t g = 0; g < pl.groups.size(); ++g) {
                if (pl.groups[g].level == lev) {
                    emit_glue_group(g, k);
                }
            }
            sync();
        }
    };

    const auto jet_off = [&](std::uint32_t k, std::uint32_t r) {
        // jetw[(k * spw + q) * n_col + r * L + l]
        return "jetl[" + std::to_string(static_cast<std::uint64_t>(k) * spw * n_col + static_cast<std::uint64_t>(r) * L)
               + "]";
    };

    // ===================== kernel body =====================
    // Order 0: publish the state.
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        os << "slab[" << utname(svr[r].out_tbl) << "] = xs" << r << ";\n";
        os << jet_off(0, r) << " = xs" << r << ";\n";
    }
    {
        std::string m = "fabs(xs0)";
        os << "double m0 = fabs(xs0);\n";
        for (std::uint32_t r = 1; r < sv_rounds; ++r) {
            os << "if (svalid" << r << ") m0 = hy_max(m0, fabs(xs" << r << "));\n";
        }
        (void)m;
    }
    sync();
    emit_levels(0);
    os << "double mo = 0.0, mom1 = 0.0;\n";
    for (std::uint32_t k = 1; k <= order; ++k) {
        // State-variable recursion: read rhs^[k-1], sync, write x^[k].
        std::vector<std::string> rhs(sv_rounds);
        for (std::uint32_t r = 0; r < sv_rounds; ++r) {
            if (svr[r].any_var) {
                rhs[r] = e.def("slab[" + utname(svr[r].in_tbl) + "]");
            }
        }
        sync();
        for (std::uint32_t r = 0; r < sv_rounds; ++r) {
            std::string xv;
            if (svr[r].any_var) {
                xv = e.def(rhs[r] + " / " + fp_literal(static_cast<double>(k)));
            } else {
                xv = (k == 1u) ? dtname(svr[r].cst_tbl) : std::string("0.0");
            }
            os << "slab[" << utname(svr[r].out_tbl) << "] = " << xv << ";\n";
            os << jet_off(k, r) << " = " << xv << ";\n";
            if (k == order - 1u || k == order) {
                const char *acc = (k == order) ? "mo" : "mom1";
                if (r == 0u) {
                    os << acc << " = fabs(" << xv << ");\n";
                } else {
                    os << "if (svalid" << r << ") " << acc << " = hy_max(" << acc << ", fabs(" << xv << "));\n";
                }
            }
        }
        sync();
        if (k < order) {
            emit_levels(k);
        }
    }
    body << os.str();
    os.str("");
    os.clear();

    // ===================== module text =====================
    std::ostringstream src;
    src << prelude() << emit_detail::step_loop_source() << (opts.angle_reduce.empty() ? "" : angle_reduce_helper_source);
    emit_detail::emit_dout(src, p, opts);

    src << emit_detail::wsync_macro;
    src << "__constant__ unsigned short hy_utbl[" << std::max<std::size_t>(utbl.size(), 1u) * L << "] = {";
    for (const auto &v : utbl) {
        for (const auto x : v) {
            src << x << ",";
        }
    }
    src << "};\n";
    src << "__constant__ double hy_dtbl[" << std::max<std::size_t>(dtbl.size(), 1u) * L << "] = {";
    for (const auto &v : dtbl) {
        for (const auto x : v) {
            src << fp_literal(x) << ",";
        }
    }
    src << "};\n";

    src << "extern \"C\" __global__ void __launch_bounds__(" << bs << ") hy_taylor(const hy_kargs a)\n{\n";
    src << "__shared__ double lds_slab[" << static_cast<std::uint64_t>(wpb) * spw * slab_stride << "];\n";
    src << "const unsigned lane = threadIdx.x & 63u;\nconst unsigned wib = threadIdx.x >> 6;\n";
    src << "const unsigned l = lane % " << L << "u;\nconst unsigned q = lane / " << L << "u;\n";
    src << "const u64 N = a.N;\n";
    src << "double *const slab = lds_slab + (wib * " << spw << "u + q) * " << slab_stride << "u;\n";
    src << "const u64 gwave = (u64)blockIdx.x * " << wpb << "u + wib;\n";
    // The jets of the state variables of the systems of a wavefront ([order][system][variable]): in LDS when they fit next to
    // the slab (round 6: one workgroup per CU runs anyway - one wavefront per SIMD -, and through global scratch they cost
    // the chain of 16 pendula 44 GB of HBM traffic per launch, 1.2 TB/s), otherwise in a per-wavefront global scratch.
    // (This kernel declares two arrays in LDS, the slab and the jets; 2 KB are kept in hand for their alignment and the
    // compiler's own use. The slab alone is held to the same limit: a plan whose slab does not fit is declined.)
    const std::uint64_t jet_doubles_per_wave = static_cast<std::uint64_t>(order + 1u) * spw * n_col;
    const std::uint64_t lds_slab_bytes = static_cast<std::uint64_t>(wpb) * spw * slab_stride * 8u, lds_limit_bytes = 160u * 1024u;
    const bool jets_in_lds = lds_slab_bytes + static_cast<std::uint64_t>(wpb) * jet_doubles_per_wave * 8u + 2048u <= lds_limit_bytes;
    if (!jets_in_lds && lds_slab_bytes + 2048u > lds_limit_bytes) {
        why_not = "the slabs of the systems of a CU (" + std::to_string(lds_slab_bytes) + " bytes) do not fit in its LDS";
        return ret;
    }
    if (jets_in_lds) {
        src << "__shared__ double lds_jets[" << static_cast<std::uint64_t>(wpb) * jet_doubles_per_wave << "];\n";
        src << "double *const jetw = lds_jets + wib * " << jet_doubles_per_wave << "u;\n";
    } else {
        src << "double *const jetw = a.scratch + gwave * " << jet_doubles_per_wave << "ull;\n";
    }
    src << "double *const jetl = jetw + q * " << n_col << "u + l;\n";
    // Per-lane table entries (loop invariant).
    for (std::size_t t = 0; t < utbl.size(); ++t) {
        src << "const unsigned ut" << t << " = hy_utbl[" << t * L << "u + l];\n";
    }
    for (std::size_t t = 0; t < dtbl.size(); ++t) {
        src << "const double dt" << t << " = hy_dtbl[" << t * L << "u + l];\n";
    }
    for (const auto &[nm, t] : cst_names) {
        src << "const double " << nm << " = dt" << t << ";\n";
    }
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        src << "const bool svalid" << r << " = (" << r * L << "u + l) < " << n_eq << "u;\n";
        src << "const unsigned svi" << r << " = svalid" << r << " ? (" << r * L << "u + l) : " << r * L << "u;\n";
    }
    // Fused callback::angle_reducer (emit_options::angle_reduce): lane l of a system holds the state variables r * L + l;
    // sred<r> says whether the one of round r is flagged (rounds without a flagged variable get no code at all).
    std::vector<char> round_reduced(sv_rounds, 0);
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        std::string cond;
        for (const auto i : opts.angle_reduce) {
            if (i / L == r) {
                cond += (cond.empty() ? "" : " || ") + ("svi" + std::to_string(r) + " == " + std::to_string(i) + "u");
            }
        }
        if (!cond.empty()) {
            round_reduced[r] = 1;
            src << "const bool sred" << r << " = svalid" << r << " && (" << cond << ");\n";
        }
    }
    ret.angle_reduce_fused = !opts.angle_reduce.empty();
    src << R"HIP(
for (;;) {
// Pull the next group of systems from the device-side work queue.
u64 base = 0;
if (lane == 0u) base = atomicAdd((u64 *)(a.counters + 2), (u64)SPW);
base = __shfl(base, 0, 64);
if (base >= N) break;
// NOTE: lanes beyond the end of the ensemble replicate the last system (no side effects).
const bool live = (base + q) < N;
const u64 s = live ? (base + q) : (N - 1u);
double t_hi = a.time_hi[s], t_lo = a.time_lo[s];
)HIP";
    for (std::uint32_t i = 0; i < p.n_par; ++i) {
        src << "const double par_" << i << " = a.pars[(u64)" << i << "u * N + s];\n";
    }
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        src << "double xs" << r << " = a.state[(u64)svi" << r << " * N + s];\n";
    }
    src << R"HIP(
HY_STEP_LIMITS(s, HY_DIR_BRANCHY)
HY_STEP_COUNTERS
for (;;) {
HY_STEP_LIM
)HIP";
    src << body.str();

    // Step size: reduce the partial maxima over the lanes of the group with wavefront shuffles.
    for (std::uint32_t m = 1; m < L; m *= 2u) {
        src << "m0 = hy_max(m0, __shfl_xor(m0, " << m << ", 64));\n";
        src << "mo = hy_max(mo, __shfl_xor(mo, " << m << ", 64));\n";
        src << "mom1 = hy_max(mom1, __shfl_xor(mom1, " << m << ", 64));\n";
    }
    src << "HY_STEP_SIZE(" << fp_literal(1. / static_cast<double>(order)) << ", " << fp_literal(1. / static_cast<double>(order - 1u))
        << ", " << fp_literal(rhofac(order)) << ")\n";

    // State update from the scratch jets.
    src << "asm volatile(\"\" ::: \"memory\");\n";
    const auto kstride = static_cast<std::uint64_t>(spw) * n_col;
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        src << "{\nconst double *c = jetl + " << static_cast<std::uint64_t>(r) * L << "u;\n";
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
        if (round_reduced[r] != 0) {
            src << "xs" << r << " = sred" << r << " ? hy_angle_red(res) : res;\n}\n";
        } else {
            src << "xs" << r << " = res;\n}\n";
        }
    }
    src << R"HIP(
HY_STEP_ADVANCE
int nfi = !(hy_finite(t_hi) && hy_finite(t_lo)) ? 1 : 0;
)HIP";
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        src << "if (svalid" << r << " && !hy_finite(xs" << r << ")) nfi = 1;\n";
    }
    for (std::uint32_t m = 1; m < L; m *= 2u) {
        src << "nfi |= __shfl_xor(nfi, " << m << ", 64);\n";
    }
    src << R"HIP(
// The coefficients of the step just taken, in the reference's layout, if requested.
if (a.tc != nullptr && live) {
)HIP";
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        src << "if (svalid" << r << ") {\nconst double *c = jetl + " << static_cast<std::uint64_t>(r) * L
            << "u;\nfor (unsigned k = 0; k <= " << order << "u; ++k) a.tc[((u64)svi" << r << " * "
            << (order + 1u) << "u + k) * N + s] = c[(u64)k * " << kstride << "u];\n}\n";
    }
    src << R"HIP(
}
HY_STEP_TAIL(nfi != 0, l == 0u && live)
}
)HIP";
    for (std::uint32_t r = 0; r < sv_rounds; ++r) {
        src << "if (svalid" << r << " && live) a.state[(u64)svi" << r << " * N + s] = xs" << r << ";\n";
    }
    src << R"HIP(
if (l == 0u && live) {
    HY_STEP_RESULT(s)
}
}
}
)HIP";

    auto text = src.str();
    // SPW macro used by the work-queue code.
    const std::string spw_def = "#define SPW " + std::to_string(spw) + "u\n";
    ret.source = spw_def + text;
    ret.kernel_name = "hy_taylor";
    ret.dout_name = "hy_dout";
    ret.block_size = bs;
    ret.lanes_per_system = L;
    ret.lds_bytes = 0;
    ret.mode = emit_mode::cluster;
    ret.cluster_generation = 1;
    ret.n_statements = e.n_stmt;
    ret.scratch_per_wave = jets_in_lds ? 0u : jet_doubles_per_wave;
    ret.persistent = true;
    ret.tc_optional = true;
    if (classes.size() == 1u) {
        ret.notes = "cluster mode: " + std::to_string(nc) + " clusters of " + std::to_string(pl.clusters[0].size()) + " nodes";
    } else {
        ret.notes = "cluster mode (" + std::to_string(classes.size()) + " classes of clusters:";
        for (const auto &cls : classes) {
            ret.notes += " " + std::to_string(cls.members.size()) + " x " + std::to_string(pl.clusters[cls.members[0]].size())
                         + " nodes at level " + std::to_string(cls.level) + ",";
        }
        ret.notes.back() = ')';
        ret.notes += ": " + std::to_string(nc) + " clusters";
    }
    ret.notes += ", L=" + std::to_string(L) + ", " + std::to_string(pl.n_slots) + " LDS slots, "
                 + std::to_string(pl.groups.size()) + " glue groups, " + std::to_string(utbl.size()) + " slot tables, jets in "
                 + (jets_in_lds ? "LDS" : "global scratch");
    (void)n_slots_tot;
    return ret;
}

// Returns a module with an empty source (and the reason in why_not) if cluster mode is not applicable.
emitted_module emit_cluster_or_empty(const taylor_program &p, const emit_options &opts, emit_refusal &why_not)
{
    if (!opts.dev.cluster_v1 && opts.cluster_kernel != 1) {
        emit_refusal why2;
        auto m = emit_cluster_v2(p, opts, why2);
        if (!m.source.empty()) {
            return m;
        }
        auto m1 = emit_cluster_v1(p, opts, why_not, false);
        if (!m1.source.empty()) {
            m1.notes += " (pipelined cluster kernel not applicable: " + why2.text + ")";
        }
        return m1;
    }
    return emit_cluster_v1(p, opts, why_not, false);
}

// Clusters of several shapes / at several dependency levels: one section of code per class (see cluster_class).
emitted_module emit_cluster_multi_or_empty(const taylor_program &p, const emit_options &opts, emit_refusal &why_not)
{
    return emit_cluster_v1(p, opts, why_not, true);
}

} // namespace heyoka_amd
