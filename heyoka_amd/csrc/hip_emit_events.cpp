// The event-side generators: the companion kernel hy_ev_jets of the wave-cluster steppers with events, the same computation as
// statements for use inside a stepper, and the matcher of the close-encounter events. See hip_emit.hpp.
#include "dense_output_text.hpp"
#include "hip_emit.hpp"
#include "hip_emit_detail.hpp"

#include <algorithm>
#include <functional>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace heyoka_amd
{

namespace
{

// The nodes the event equations need - the transitive closure over the arguments and the hidden dependencies -, how often
// each u variable is read (by a needed node or as an event equation) and the number of needed nodes (the state variables not
// counted). skip_events (optional, one flag per event equation): equations which are left out.
struct ev_closure {
    std::vector<char> need;
    std::vector<std::uint32_t> uses;
    std::uint32_t n_nodes = 0;
};

ev_closure event_closure(const taylor_program &p, const std::vector<char> *skip_events)
{
    ev_closure c{std::vector<char>(p.n_u, 0), std::vector<std::uint32_t>(p.n_u, 0), 0};
    const auto mark = [&](std::uint32_t u) {
        c.need[u] = 1;
        ++c.uses[u];
    };
    for (std::size_t ev = 0; ev < p.ev_u.size(); ++ev) {
        if (skip_events == nullptr || (*skip_events)[ev] == 0) {
            mark(p.ev_u[ev]);
        }
    }
    for (std::uint32_t u = p.n_u; u-- > p.n_eq;) {
        if (c.need[u] == 0) {
            continue;
        }
        ++c.n_nodes;
        const auto &n = p.nodes[u - p.n_eq];
        for (const auto &o : n.args) {
            if (o.type == operand::kind::uvar) {
                mark(o.idx);
            }
        }
        for (const auto d : n.deps) {
            mark(d);
        }
    }
    return c;
}

} // namespace

// Jets of the event equations from the jets of the state variables (see hip_emit.hpp). The part of the decomposition the
// event equations depend on is run order by order, one system per lane, with the coefficients of the state variables
// loaded from a.tc instead of being produced by the recursion x^[k+1] = f^[k] / (k + 1) - the elementary-function rules
// (and hence the coefficients) are the ones of the stepper with events of the one-system-per-lane kernels. The norms of
// the step-size selector are those of the state variables (a.sel_norms, written by the cluster stepper in mode 4)
// extended to the event equations (taylor_determine_h() iterates up to n_eq + n_sv_funcs, src/taylor_00.cpp:209-219).
emitted_module emit_event_jets(const taylor_program &p, const emit_options &opts, std::string &why_not)
{
    using emit_detail::ssa_emitter;
    emitted_module ret;
    const auto n_eq = p.n_eq;
    const auto order = opts.order;
    if (p.ev_u.empty()) {
        why_not = "no event equations";
        return ret;
    }
    const auto closure = event_closure(p, nullptr);
    const auto &need = closure.need;
    const auto n_nodes = closure.n_nodes;
    const auto n_sv = static_cast<std::uint32_t>(std::count(need.begin(), need.begin() + n_eq, 1));
    // NOTE: straight-line code with the histories in registers, like the unrolled stepper.
    const std::uint32_t max_nodes = 40;
    if (n_nodes > max_nodes) {
        why_not = "the event equations depend on " + std::to_string(n_nodes) + " nodes of the decomposition (limit: "
                  + std::to_string(max_nodes) + ")";
        return ret;
    }

    // Compact Taylor coefficients (emit_options::compact_tc): the stepper wrote only the order-0 row of the state
    // variables defined by another state variable; their higher orders are parent^[k-1] / k - a multiplication by
    // RN(1 / k) like the state recursion of the pair kernels, the correctly rounded quotient under kw::exact_division.
    const auto rows = emit_detail::make_compact_rows(p, opts);
    const auto derived_coeff = [&](const std::string &parent, std::uint32_t k) {
        return emit_detail::derived_coeff_text(opts, parent, fp_literal(emit_detail::rk_value(opts, k)));
    };

    ssa_emitter e(p, order);
    auto &os = e.os;
    // (The same node rules and addition order as the one-system-per-lane stepper with events.)
    e.running_sums = opts.sum_order != 1;
    if (opts.compact_tc) {
        // (The kernels which serve the compact coefficients travel in this module: hy_dout_c, hy_tc_expand.)
        os << emit_detail::compact_tc_kernels_text(p, opts);
    }
    os << "extern \"C\" __global__ void __launch_bounds__(256) hy_ev_jets(const hy_kargs a)\n{\n";
    os << "const u64 N = a.N;\nconst u64 s = (u64)blockIdx.x * 256u + threadIdx.x;\nif (s >= N) return;\n";
    std::vector<char> par_used(p.n_par, 0);
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (need[u] != 0) {
            for (const auto &o : p.nodes[u - n_eq].args) {
                if (o.type == operand::kind::par) {
                    par_used[o.idx] = 1;
                }
            }
        }
    }
    for (std::uint32_t i = 0; i < p.n_par; ++i) {
        if (par_used[i] != 0) {
            os << "const double par_" << i << " = a.pars[(u64)" << i << "u * N + s];\n";
        }
    }
    os << "const double *const jet = a.tc + s;\n";
    // (The order-0 rule of func_kind::time reads the time coordinate by this name: an event equation like time - 0.5.)
    os << "const double t_hi = a.time_hi[s];\n(void)t_hi;\n";
    for (std::uint32_t k = 0; k <= order; ++k) {
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            if (need[i] != 0) {
                if (rows.derived(i) && k > 0u) {
                    // (Compact Taylor coefficients: x^[k] = v^[k-1] / k with the arithmetic of the stepper.)
                    e.val(i, k) = e.def(derived_coeff("jet[(u64)"
                                                          + std::to_string(static_cast<std::uint64_t>(p.sv_defs[i].idx) * (order + 1u)
                                                                           + (k - 1u))
                                                          + "u * N]",
                                                      k));
                } else {
                    e.val(i, k)
                        = e.def("jet[(u64)" + std::to_string(static_cast<std::uint64_t>(i) * (order + 1u) + k) + "u * N]");
                }
            }
        }
        for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
            if (need[u] != 0) {
                e.node(u - n_eq, k);
            }
        }
        for (std::size_t ev = 0; ev < p.ev_u.size(); ++ev) {
            os << "a.ev_tc[(u64)" << (ev * (order + 1u) + k) << "u * N + s] = " << e.val(p.ev_u[ev], k) << ";\n";
        }
    }
    // Norms: state variables first, then the event equations, combined like the pairwise maximum of the stepper with
    // events (the maximum of non-NaN values does not depend on the order of the comparisons).
    const auto ext = [&](const std::string &base, std::uint32_t k) {
        auto m = e.def(base);
        for (const auto u : p.ev_u) {
            m = e.def("hy_max(" + m + ", fabs(" + e.val(u, k) + "))");
        }
        return m;
    };
    const auto m0 = ext("a.sel_norms[s]", 0), mo = ext("a.sel_norms[N + s]", order), mom1 = ext("a.sel_norms[2u * N + s]", order - 1u);
    os << "const double num_rho = (" << m0 << " <= 1.0) ? 1.0 : " << m0 << ";\n";
    os << "const double rho_o = hy_root(num_rho / " << mo << ", " << fp_literal(1. / static_cast<double>(order)) << ");\n";
    os << "const double rho_om1 = hy_root(num_rho / " << mom1 << ", " << fp_literal(1. / static_cast<double>(order - 1u))
       << ");\n";
    os << "const double rho_m = hy_min(rho_o, rho_om1);\n";
    os << "double h = rho_m * " << fp_literal(emit_detail::rhofac(order)) << ";\n";
    os << "const double lim = a.lim[s];\nh = hy_min(h, fabs(lim));\nh = (lim < 0.0) ? -h : h;\n";
    os << "a.last_h[s] = h;\na.max_abs_state[s] = " << m0 << ";\n}\n";

    std::ostringstream src;
    src << emit_detail::prelude() << emit_detail::rules_source(p) << os.str();
    ret.source = src.str();
    ret.kernel_name = "hy_ev_jets";
    ret.block_size = 256;
    ret.lanes_per_system = 1;
    ret.mode = emit_mode::unrolled;
    ret.n_statements = e.n_stmt;
    ret.notes = "jets of " + std::to_string(p.ev_u.size()) + " event equation(s) from the jets of " + std::to_string(n_sv)
                + " state variable(s), " + std::to_string(n_nodes) + " nodes";
    return ret;
}

bool emit_event_jets_inline(const taylor_program &p, const emit_options &opts,
                            const std::function<std::string(std::uint32_t, std::uint32_t)> &sv,
                            const std::function<std::string(std::uint32_t, std::uint32_t, const std::string &)> &ev_store,
                            std::string &out, std::vector<std::vector<std::string>> &ev_coeffs, std::string &why_not,
                            ev_lane_hooks *lanes, const std::vector<char> *skip_events)
{
    using emit_detail::ssa_emitter;
    const auto n_eq = p.n_eq;
    const auto order = opts.order;
    if (p.ev_u.empty()) {
        why_not = "no event equations";
        return false;
    }
    const auto skipped_ev = [&](std::size_t ev) { return skip_events != nullptr && (*skip_events)[ev] != 0; };
    const auto closure = event_closure(p, skip_events);
    const auto &need = closure.need;
    const auto &uses = closure.uses;
    const auto n_nodes = closure.n_nodes;
    // What the statements inside a stepper cannot serve - the first offence from the last needed node down, as the closure
    // meets them (everything which reads a node comes after it).
    for (std::uint32_t u = p.n_u; u-- > n_eq;) {
        if (need[u] == 0) {
            continue;
        }
        const auto &n = p.nodes[u - n_eq];
        if (n.kind == func_kind::custom) {
            why_not = "an event equation depends on a function defined through a node rule";
            return false;
        }
        if (std::any_of(n.args.begin(), n.args.end(), [](const auto &o) { return o.type == operand::kind::par; })) {
            why_not = "an event equation depends on a runtime parameter";
            return false;
        }
    }

    // Sums of isomorphic terms (ev_lane_hooks): which needed nodes are evaluated by lane c of the system for term c. A sum
    // written with binary operators arrives as a chain, sum(sum(t0, t1), t2): a later sum which adds more terms of the same
    // shape to the result of an earlier one extends its group.
    struct lane_group {
        std::vector<std::uint32_t> roots;               // root of term c
        std::vector<std::uint32_t> nodes0;              // nodes of term 0 (ascending)
        std::vector<std::vector<std::uint32_t>> leaves; // [c][p]: state variable at leaf position p of term c
        std::string sig;
        // sum node -> (argument position, term) pairs it collects
        std::map<std::uint32_t, std::vector<std::pair<std::uint32_t, std::uint32_t>>> collect;
        std::uint32_t last_sum = 0;
    };
    std::vector<lane_group> groups;
    std::vector<int> owner(p.n_u, -1);   // group of a node which belongs to a term (roots included)
    std::vector<char> skipped(p.n_u, 0); // nodes of the terms c >= 1: never emitted
    if (lanes != nullptr) {
        lanes->leaf_vars.clear();
        lanes->leaf_class.clear();
        std::vector<std::vector<std::uint32_t>> claimed; // nodes of all the terms accepted so far
        const auto linear_node = [&](const dc_node &n) {
            return n.kind == func_kind::sum || n.kind == func_kind::sub
                   || (n.kind == func_kind::prod
                       && std::any_of(n.args.begin(), n.args.end(), [](const auto &o) { return o.type != operand::kind::uvar; }));
        };
        for (std::uint32_t S = n_eq; S < p.n_u; ++S) {
            const auto &ns = p.nodes[S - n_eq];
            const auto m = static_cast<std::uint32_t>(ns.args.size());
            if (need[S] == 0 || ns.kind != func_kind::sum || m < 2u) {
                continue;
            }
            bool ok = true;
            int ext = -1; // the group whose running sum is one of the arguments
            std::vector<std::uint32_t> cand_pos;
            for (std::uint32_t a = 0; ok && a < m; ++a) {
                const auto &o = ns.args[a];
                ok = ok && o.type == operand::kind::uvar && o.idx >= n_eq && uses[o.idx] == 1u;
                if (!ok) {
                    break;
                }
                int gs = -1;
                for (std::size_t gi = 0; gi < groups.size(); ++gi) {
                    if (groups[gi].last_sum == o.idx) {
                        gs = static_cast<int>(gi);
                    }
                }
                if (gs >= 0) {
                    ok = ok && ext < 0;
                    ext = gs;
                } else {
                    ok = ok && owner[o.idx] < 0;
                    cand_pos.push_back(a);
                }
                for (std::uint32_t b = a + 1u; b < m; ++b) {
                    ok = ok && ns.args[a].idx != ns.args[b].idx;
                }
            }
            const auto n_old = ext >= 0 ? static_cast<std::uint32_t>(groups[static_cast<std::size_t>(ext)].roots.size()) : 0u;
            ok = ok && !cand_pos.empty() && (ext >= 0 || cand_pos.size() >= 2u) && n_old + cand_pos.size() <= lanes->max_terms;
            if (!ok) {
                continue;
            }
            std::vector<std::string> sigs;
            std::vector<std::vector<std::uint32_t>> term_nodes, term_leaves;
            for (std::size_t ci = 0; ok && ci < cand_pos.size(); ++ci) {
                const auto root = ns.args[cand_pos[ci]].idx;
                std::vector<std::uint32_t> nodes, leaves;
                std::map<std::uint32_t, std::uint32_t> refs; // references to the nodes of the term from inside it
                const std::function<std::string(std::uint32_t)> sig = [&](std::uint32_t u) -> std::string {
                    if (u < n_eq) {
                        auto it = std::find(leaves.begin(), leaves.end(), u);
                        if (it == leaves.end()) {
                            leaves.push_back(u);
                            it = leaves.end() - 1;
                        }
                        return "s" + std::to_string(lanes->sv_class(u)) + ":" + std::to_string(it - leaves.begin());
                    }
                    ++refs[u];
                    if (const auto it = std::find(nodes.begin(), nodes.end(), u); it != nodes.end()) {
                        return "r" + std::to_string(it - nodes.begin());
                    }
                    const auto &n = p.nodes[u - n_eq];
                    if (!n.deps.empty() || n.kind == func_kind::time || owner[u] >= 0) {
                        ok = false;
                        return "";
                    }
                    nodes.push_back(u);
                    std::string r = std::string(func_kind_name(n.kind)) + "[";
                    for (const auto &o : n.args) {
                        if (o.type == operand::kind::par) {
                            ok = false;
                        }
                        r += (o.type == operand::kind::num) ? ("n" + fp_literal(o.value)) : sig(o.idx);
                        r += ",";
                    }
                    return r + "]";
                };
                sigs.push_back(sig(root));
                // Nothing outside the term reads its nodes (the reference of the sum to the root is the first call of sig()).
                for (const auto u : nodes) {
                    ok = ok && uses[u] == refs[u];
                }
                // (Terms are disjoint.)
                for (const auto *lst : {&claimed, &term_nodes}) {
                    for (const auto &tn : *lst) {
                        for (const auto u : nodes) {
                            ok = ok && std::find(tn.begin(), tn.end(), u) == tn.end();
                        }
                    }
                }
                const auto &ref_sig = ext >= 0 ? groups[static_cast<std::size_t>(ext)].sig : sigs[0];
                ok = ok && sigs.back() == ref_sig && !leaves.empty();
                std::sort(nodes.begin(), nodes.end());
                term_nodes.push_back(std::move(nodes));
                term_leaves.push_back(std::move(leaves));
            }
            // A term without a convolution is not worth the lane broadcasts.
            bool has_conv = ext >= 0;
            if (ok && ext < 0) {
                for (const auto u : term_nodes[0]) {
                    has_conv = has_conv || !linear_node(p.nodes[u - n_eq]);
                }
            }
            if (!ok || !has_conv) {
                continue;
            }
            if (ext < 0) {
                groups.emplace_back();
                ext = static_cast<int>(groups.size()) - 1;
                groups.back().sig = sigs[0];
                groups.back().nodes0 = term_nodes[0];
            }
            auto &g = groups[static_cast<std::size_t>(ext)];
            for (std::size_t ci = 0; ci < cand_pos.size(); ++ci) {
                const auto c = static_cast<std::uint32_t>(g.roots.size());
                for (const auto u : term_nodes[ci]) {
                    owner[u] = ext;
                    skipped[u] = c >= 1u ? 1 : 0;
                }
                g.roots.push_back(ns.args[cand_pos[ci]].idx);
                g.leaves.push_back(term_leaves[ci]);
                g.collect[S].emplace_back(cand_pos[ci], c);
                claimed.push_back(term_nodes[ci]);
            }
            g.last_sum = S;
        }
    }

    // NOTE: every lane of a system runs these statements (the wavefront of the one-lane-per-pair kernel holds FOUR systems
    // where hy_ev_jets holds 64: a convolution costs 16 times the lane-time here). What the stepper saves is the
    // dense-output pass over the Taylor coefficients and the launch of hy_ev_jets, ~1.1 ms per 1 048 576 outer-SS systems; one
    // nonlinear node (a convolution per order: ~230 multiply-adds) costs ~0.3 ms on that scale. The budget: three nonlinear
    // nodes, any number of linear ones (coordinates, differences, sums, multiples, the time: practically free); the terms
    // of a sum which the lanes evaluate side by side count once (a squared distance AND a radial velocity fit).
    std::uint32_t n_nonlin = 0;
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (need[u] == 0 || skipped[u] != 0) {
            continue;
        }
        const auto &n = p.nodes[u - n_eq];
        bool linear = n.kind == func_kind::sum || n.kind == func_kind::sub || n.kind == func_kind::time;
        if (n.kind == func_kind::prod) {
            linear = std::any_of(n.args.begin(), n.args.end(), [](const auto &o) { return o.type != operand::kind::uvar; });
        }
        n_nonlin += linear ? 0u : (n.kind == func_kind::sum_sq ? static_cast<std::uint32_t>((n.args.size() + 1u) / 2u) : 1u);
    }
    std::uint32_t max_nonlin = 3, max_nodes = 40;
    if (opts.dev.ev_inline_max_nonlinear >= 0) {
        max_nonlin = static_cast<std::uint32_t>(opts.dev.ev_inline_max_nonlinear);
        max_nodes = std::max(max_nodes, 12u * max_nonlin);
    }
    if (n_nonlin > max_nonlin || n_nodes > max_nodes) {
        why_not = "the event equations depend on " + std::to_string(n_nonlin) + " nonlinear / " + std::to_string(n_nodes)
                  + " nodes of the decomposition (budget inside the stepper: " + std::to_string(max_nonlin) + " / "
                  + std::to_string(max_nodes) + ")";
        return false;
    }

    // Leaf positions of the groups, globally numbered; state variables which are (also) read outside the terms.
    std::vector<std::uint32_t> leaf_base(groups.size(), 0);
    for (std::size_t gi = 0; gi < groups.size(); ++gi) {
        leaf_base[gi] = static_cast<std::uint32_t>(lanes->leaf_vars.size());
        const auto &g = groups[gi];
        for (std::size_t pp = 0; pp < g.leaves[0].size(); ++pp) {
            std::vector<std::uint32_t> vars;
            for (const auto &lv : g.leaves) {
                vars.push_back(lv[pp]);
            }
            lanes->leaf_class.push_back(lanes->sv_class(vars[0]));
            lanes->leaf_vars.push_back(std::move(vars));
        }
    }
    std::vector<char> scalar_use(n_eq, 0);
    for (std::size_t ev = 0; ev < p.ev_u.size(); ++ev) {
        if (p.ev_u[ev] < n_eq && !skipped_ev(ev)) {
            scalar_use[p.ev_u[ev]] = 1;
        }
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (need[u] != 0 && owner[u] < 0) {
            for (const auto &o : p.nodes[u - n_eq].args) {
                if (o.type == operand::kind::uvar && o.idx < n_eq) {
                    scalar_use[o.idx] = 1;
                }
            }
        }
    }

    ssa_emitter e(p, order);
    // (Names of their own: the statements are pasted into the body of another generator.)
    e.counter = 1000000000ull;
    // (The node rules and addition order of hy_ev_jets.)
    e.running_sums = opts.sum_order != 1;
    // lane_vals[position][k]: coefficient k of the state variable this lane holds at a leaf position.
    std::vector<std::vector<std::string>> lane_vals(lanes != nullptr ? lanes->leaf_vars.size() : 0u,
                                                    std::vector<std::string>(order + 1u));
    // (What this lane computed for its term, by group and order: read by every sum of the chain which collects terms.)
    std::vector<std::vector<std::string>> own_val(groups.size(), std::vector<std::string>(order + 1u));
    const auto swap_leaves = [&](const lane_group &g, std::uint32_t base, std::uint32_t k) {
        for (std::size_t pp = 0; pp < g.leaves[0].size(); ++pp) {
            for (std::uint32_t j = 0; j <= k; ++j) {
                std::swap(e.val(g.leaves[0][pp], j), lane_vals[base + pp][j]);
            }
        }
    };
    for (std::uint32_t k = 0; k <= order; ++k) {
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            if (need[i] != 0 && scalar_use[i] != 0) {
                e.val(i, k) = e.def(sv(i, k));
            }
        }
        for (std::size_t pp = 0; pp < lane_vals.size(); ++pp) {
            lane_vals[pp][k] = e.def(lanes->sv_lane(static_cast<std::uint32_t>(pp), k, lanes->leaf_class[pp]));
        }
        for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
            if (need[u] == 0 || skipped[u] != 0) {
                continue;
            }
            if (owner[u] >= 0) {
                // A node of term 0 of a group: evaluated by every lane on ITS term's state variables.
                const auto gi = static_cast<std::size_t>(owner[u]);
                swap_leaves(groups[gi], leaf_base[gi], k);
                e.node(u - n_eq, k);
                swap_leaves(groups[gi], leaf_base[gi], k);
                continue;
            }
            for (auto &g : groups) {
                if (const auto it = g.collect.find(u); it != g.collect.end()) {
                    // The terms in the order of the arguments: the value of term c is what lane c computed.
                    if (own_val[&g - groups.data()][k].empty()) {
                        own_val[&g - groups.data()][k] = e.val(g.roots[0], k);
                    }
                    for (const auto &[pos, c] : it->second) {
                        (void)pos;
                        e.val(g.roots[c], k) = e.def(lanes->lane_bcast(own_val[&g - groups.data()][k], c));
                    }
                }
            }
            e.node(u - n_eq, k);
        }
        for (std::size_t ev = 0; ev < p.ev_u.size(); ++ev) {
            if (!skipped_ev(ev)) {
                e.os << ev_store(static_cast<std::uint32_t>(ev), k, e.val(p.ev_u[ev], k));
            }
        }
    }
    ev_coeffs.clear();
    for (std::size_t ev = 0; ev < p.ev_u.size(); ++ev) {
        std::vector<std::string> c;
        for (std::uint32_t k = 0; !skipped_ev(ev) && k <= order; ++k) {
            c.push_back(e.val(p.ev_u[ev], k));
        }
        ev_coeffs.push_back(std::move(c));
    }
    out = e.os.str();
    return true;
}

bool match_pair_distance_event(const taylor_program &p, std::uint32_t u, pair_distance_event &out)
{
    const auto n_eq = p.n_eq;
    if (u < n_eq) {
        return false;
    }
    // Flatten the sums / differences at the top: squares and numeric constants.
    std::vector<std::uint32_t> sq_args; // the u variable whose square a term is
    std::vector<bool> sq_neg;           // ... and whether the square is subtracted
    double c = 0;
    bool ok = true;
    const std::function<void(std::uint32_t, bool)> term = [&](std::uint32_t v, bool negated) {
        if (!ok || v < n_eq) {
            ok = false;
            return;
        }
        const auto &n = p.nodes[v - n_eq];
        const auto arg = [&](const operand &o, bool neg) {
            if (o.type == operand::kind::num) {
                c += neg ? -o.value : o.value;
            } else if (o.type == operand::kind::uvar) {
                term(o.idx, neg);
            } else {
                ok = false;
            }
        };
        if (n.kind == func_kind::sum) {
            for (const auto &o : n.args) {
                arg(o, negated);
            }
        } else if (n.kind == func_kind::sub && n.args.size() == 2u) {
            arg(n.args[0], negated);
            arg(n.args[1], !negated);
        } else if (n.kind == func_kind::prod && n.args.size() == 2u && n.args[0].type == operand::kind::num
                   && n.args[0].value == -1. && n.args[1].type == operand::kind::uvar) {
            // (-x is written as -1 * x.)
            term(n.args[1].idx, !negated);
        } else if (n.kind == func_kind::prod && n.args.size() == 2u && n.args[0].type == operand::kind::uvar
                   && n.args[1].type == operand::kind::uvar && n.args[0].idx == n.args[1].idx) {
            sq_args.push_back(n.args[0].idx);
            sq_neg.push_back(negated);
        } else if (n.kind == func_kind::pow && n.args.size() == 2u && n.args[0].type == operand::kind::uvar
                   && n.args[1].type == operand::kind::num && n.args[1].value == 2.) {
            sq_args.push_back(n.args[0].idx);
            sq_neg.push_back(negated);
        } else if (n.kind == func_kind::sum_sq) {
            for (const auto &o : n.args) {
                if (o.type == operand::kind::uvar) {
                    sq_args.push_back(o.idx);
                    sq_neg.push_back(negated);
                } else {
                    ok = false;
                }
            }
        } else {
            ok = false;
        }
    };
    term(u, false);
    if (!ok || sq_args.size() != 3u || sq_neg[0] != sq_neg[1] || sq_neg[0] != sq_neg[2]) {
        return false;
    }
    out.sign = sq_neg[0] ? -1. : 1.;
    for (std::size_t i = 0; i < 3u; ++i) {
        const auto d = sq_args[i];
        if (d < n_eq) {
            return false;
        }
        const auto &n = p.nodes[d - n_eq];
        if (n.kind != func_kind::sub || n.args.size() != 2u || n.args[0].type != operand::kind::uvar
            || n.args[1].type != operand::kind::uvar || n.args[0].idx >= n_eq || n.args[1].idx >= n_eq) {
            return false;
        }
        out.diffs[i] = {n.args[0].idx, n.args[1].idx};
    }
    out.c = c;
    return true;
}

} // namespace heyoka_amd
