// The planner of the cluster code generators (hip_emit_cluster_plan.hpp): partitions a decomposition into clusters -
// connected components under "history" edges - and glue, and checks that the clusters have the shape the kernels need. A
// refusal carries a refusal_code for the reasons emit_hip_module() (hip_emit_select.cpp) and pad_clusters() react to.
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <limits>
#include <map>
#include <numeric>
#include <set>

#include "hip_emit_cluster_plan.hpp"

namespace heyoka_amd
{

std::vector<std::uint32_t> cluster_detail::history_operands(const dc_node &n, const std::vector<char> *cu)
{
    std::vector<std::uint32_t> ret;
    const auto &a = n.args;
    switch (n.kind) {
        case func_kind::prod:
            if (a.size() == 2u && is_var(a[0]) && is_var(a[1])) {
                if (cu != nullptr && ((*cu)[a[0].idx] != 0 || (*cu)[a[1].idx] != 0)) {
                    break;
                }
                ret = {a[0].idx, a[1].idx};
            }
            break;
        case func_kind::div:
            if (is_var(a[1])) {
                ret = {a[1].idx};
            }
            break;
        case func_kind::sum_sq:
            for (const auto &o : a) {
                if (is_var(o)) {
                    ret.push_back(o.idx);
                }
            }
            break;
        case func_kind::pow:
            // NOTE: sqrt only needs the current order of its base, but it always needs its own history:
            // keep things simple and treat the base as a history operand in all cases.
            if (is_var(a[0])) {
                ret = {a[0].idx};
            }
            break;
        case func_kind::sin:
        case func_kind::cos:
            if (is_var(a[0])) {
                ret = {a[0].idx};
                for (const auto d : n.deps) {
                    ret.push_back(d);
                }
            }
            break;
        case func_kind::exp:
        case func_kind::log:
            if (is_var(a[0])) {
                ret = {a[0].idx};
            }
            break;
        case func_kind::tan:
        case func_kind::tanh:
        case func_kind::sinh:
        case func_kind::cosh:
        case func_kind::erf:
        case func_kind::sigmoid:
        case func_kind::asin:
        case func_kind::acos:
        case func_kind::atan:
        case func_kind::asinh:
        case func_kind::acosh:
        case func_kind::atanh:
            // Argument + hidden dependency (the functions' own histories are added by the planner).
            if (is_var(a[0])) {
                ret = {a[0].idx};
                for (const auto d : n.deps) {
                    ret.push_back(d);
                }
            }
            break;
        default:
            break;
    }
    return ret;
}

namespace
{

using cluster_detail::cluster_plan;
using cluster_detail::glue_group;
using cluster_detail::history_operands;
using cluster_detail::is_var;

// Kinds that can be evaluated as glue (only current-order operand values).
bool is_glue_kind(const dc_node &n, const std::vector<char> *cu = nullptr)
{
    switch (n.kind) {
        case func_kind::sum:
        case func_kind::sub:
        case func_kind::num_identity:
        case func_kind::time:
            return true;
        case func_kind::prod:
            if (n.args.size() == 2u && is_var(n.args[0]) && is_var(n.args[1])) {
                return cu != nullptr && ((*cu)[n.args[0].idx] != 0 || (*cu)[n.args[1].idx] != 0);
            }
            return n.args.size() == 2u;
        case func_kind::div:
            return !is_var(n.args[1]);
        default:
            return history_operands(n, cu).empty();
    }
}

struct union_find {
    std::vector<std::uint32_t> p;
    explicit union_find(std::size_t n) : p(n)
    {
        std::iota(p.begin(), p.end(), 0u);
    }
    std::uint32_t find(std::uint32_t x)
    {
        while (p[x] != x) {
            p[x] = p[p[x]];
            x = p[x];
        }
        return x;
    }
    void unite(std::uint32_t a, std::uint32_t b)
    {
        a = find(a);
        b = find(b);
        if (a != b) {
            p[std::max(a, b)] = std::min(a, b);
        }
    }
};

// Second half of make_plan_impl() for multi-class plans: the clusters are grouped into classes of identical shape and
// dependency level; constants, exported members and histories are per class; LDS slots and glue groups as usual.
emit_refusal finish_multi_class_plan(const taylor_program &p, std::uint32_t order, cluster_plan &pl, const std::vector<char> *cu,
                                     const std::vector<std::uint32_t> &clvl, const std::vector<std::string> &sigs,
                                     const std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> &num_pos,
                                     const std::vector<std::vector<double>> &num_val, const std::vector<char> &exported)
{
    using cluster_detail::cluster_class;
    using cluster_detail::glue_group;
    const auto n_eq = p.n_eq, n_u = p.n_u;
    const auto nc = pl.clusters.size();
    // Classes, in the order of their first cluster.
    std::map<std::pair<std::uint32_t, std::string>, std::size_t> cidx;
    for (std::size_t c = 0; c < nc; ++c) {
        const auto key = std::make_pair(clvl[c], sigs[c]);
        auto it = cidx.find(key);
        if (it == cidx.end()) {
            it = cidx.emplace(key, pl.classes.size()).first;
            pl.classes.emplace_back();
            pl.classes.back().level = clvl[c];
        }
        pl.classes[it->second].members.push_back(static_cast<std::uint32_t>(c));
    }
    std::size_t max_members = 0, stored_total = 0;
    for (auto &cls : pl.classes) {
        const auto c0 = cls.members[0];
        const auto &t0 = pl.clusters[c0];
        max_members = std::max(max_members, cls.members.size());
        // Constants: literal if identical across the class, otherwise a per-lane table entry.
        cls.cst_val.assign(cls.members.size(), {});
        for (std::size_t j = 0; j < num_pos[c0].size(); ++j) {
            bool same = true;
            for (const auto c : cls.members) {
                const auto a = num_val[c][j], b = num_val[c0][j];
                if (!(a == b || (std::isnan(a) && std::isnan(b))) || std::signbit(a) != std::signbit(b)) {
                    same = false;
                }
            }
            if (!same) {
                cls.cst_pos.push_back(num_pos[c0][j]);
                for (std::size_t m = 0; m < cls.members.size(); ++m) {
                    cls.cst_val[m].push_back(num_val[cls.members[m]][j]);
                }
            }
        }
        for (std::uint32_t q = 0; q < t0.size(); ++q) {
            bool any = false;
            for (const auto c : cls.members) {
                any = any || exported[pl.clusters[c][q]] != 0;
            }
            if (any) {
                cls.out_pos.push_back(q);
            }
        }
        // Histories of the template.
        std::set<std::uint32_t> stored;
        for (const auto u : t0) {
            const auto &n = p.nodes[u - n_eq];
            const auto hs = history_operands(n, cu);
            for (const auto h : hs) {
                stored.insert(h);
            }
            switch (n.kind) {
                case func_kind::pow:
                case func_kind::div:
                case func_kind::sin:
                case func_kind::cos:
                case func_kind::exp:
                case func_kind::log:
                case func_kind::sigmoid:
                case func_kind::asin:
                case func_kind::acos:
                case func_kind::atan:
                case func_kind::asinh:
                case func_kind::acosh:
                case func_kind::atanh:
                    if (!hs.empty()) {
                        stored.insert(u);
                    }
                    break;
                default:
                    break;
            }
        }
        for (std::uint32_t q = 0; q < t0.size(); ++q) {
            if (stored.count(t0[q]) != 0u) {
                cls.stored_pos.push_back(q);
            }
        }
        stored_total += stored.size();
    }
    if (max_members > 64u) {
        return "more than 64 clusters in a class";
    }
    // (Every lane carries the histories of one cluster of EVERY class.)
    if (stored_total * order * 2u > 420u) {
        return "the jets of the cluster classes do not fit in the register file (" + std::to_string(stored_total) + " histories)";
    }
    pl.L = 2;
    while (pl.L < max_members && pl.L < 64u) {
        pl.L *= 2u;
    }
    pl.spw = 64u / pl.L;
    pl.max_level = *std::max_element(pl.lvl.begin(), pl.lvl.end());

    // LDS slots: state variables, exported cluster members (output-major inside a class), glue nodes.
    pl.slot_of.assign(n_u, -1);
    std::uint32_t ns = 0;
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        pl.slot_of[i] = static_cast<int>(ns++);
    }
    for (const auto &cls : pl.classes) {
        for (const auto q : cls.out_pos) {
            for (const auto c : cls.members) {
                pl.slot_of[pl.clusters[c][q]] = static_cast<int>(ns++);
            }
        }
    }
    for (std::uint32_t u = n_eq; u < n_u; ++u) {
        if (pl.cluster_of[u] == -1) {
            pl.slot_of[u] = static_cast<int>(ns++);
        }
    }
    pl.n_slots = ns;

    // Glue groups: per level, per shape.
    const auto structural_number = [](const dc_node &n, std::size_t a) {
        if (n.kind == func_kind::pow && a == 1u) {
            return true;
        }
        return n.kind == func_kind::prod && a == 0u && n.args[0].type == operand::kind::num && n.args[0].value == -1.;
    };
    std::map<std::pair<std::uint32_t, std::string>, std::size_t> gidx;
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        const auto u = n_eq + i;
        if (pl.cluster_of[u] != -1) {
            continue;
        }
        const auto &n = p.nodes[i];
        std::ostringstream key;
        key << func_kind_name(n.kind);
        for (std::size_t a = 0; a < n.args.size(); ++a) {
            const auto &o = n.args[a];
            if (is_var(o)) {
                key << ((cu != nullptr && n.kind == func_kind::prod && (*cu)[o.idx] != 0) ? "k" : "v");
            } else if (o.type == operand::kind::par) {
                key << "p" << o.idx;
            } else if (structural_number(n, a)) {
                key << "n" << fp_literal(o.value);
            } else {
                key << "c";
            }
        }
        const auto k = std::make_pair(pl.lvl[u], key.str());
        auto it = gidx.find(k);
        if (it == gidx.end()) {
            it = gidx.emplace(k, pl.groups.size()).first;
            pl.groups.emplace_back();
            pl.groups.back().level = pl.lvl[u];
            pl.groups.back().key = key.str();
        }
        pl.groups[it->second].nodes.push_back(u);
    }
    std::stable_sort(pl.groups.begin(), pl.groups.end(),
                     [](const glue_group &a, const glue_group &b) { return a.level < b.level; });
    return {};
}

} // namespace

emit_refusal cluster_detail::make_plan_impl(const taylor_program &p, std::uint32_t order, cluster_plan &pl,
                                           const cluster_detail::plan_limits &lim)
{
    using cluster_detail::glue_group;
    const auto n_eq = p.n_eq, n_u = p.n_u;
    for (const auto &n : p.nodes) {
        if (n.kind == func_kind::custom) {
            return "functions defined through node rules run on the straight-line and interpreted steppers";
        }
    }
    pl.n_eq = n_eq;
    pl.n_u = n_u;
    // Constant u variables: only the wave-cluster generators (ssa_emitter-based) evaluate products with a constant
    // factor linearly; the block planner keeps the general treatment.
    const auto cu_store = constant_uvars(p);
    const std::vector<char> *cu = lim.jets_in_registers ? &cu_store : nullptr;

    // 1. History edges -> clusters.
    union_find uf(n_u);
    std::vector<char> in_h(n_u, 0);
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        if (p.nodes[i].kind >= func_kind::atan2) {
            // atan2, kepE and the piecewise functions: served by the unrolled / table steppers.
            return std::string("function served by the unrolled / table steppers: ") + func_kind_name(p.nodes[i].kind);
        }
        const auto u = n_eq + i;
        const auto hs = history_operands(p.nodes[i], cu);
        for (const auto h : hs) {
            if (h < n_eq) {
                return {refusal_code::state_var_history, "a state variable is a history operand of a nonlinear function"};
            }
            uf.unite(u, h);
            in_h[u] = 1;
            in_h[h] = 1;
        }
    }
    pl.cluster_of.assign(n_u, -1);
    std::map<std::uint32_t, int> root_to_cluster;
    for (std::uint32_t u = n_eq; u < n_u; ++u) {
        if (in_h[u] == 0) {
            continue;
        }
        const auto r = uf.find(u);
        auto it = root_to_cluster.find(r);
        if (it == root_to_cluster.end()) {
            it = root_to_cluster.emplace(r, static_cast<int>(pl.clusters.size())).first;
            pl.clusters.emplace_back();
        }
        pl.cluster_of[u] = it->second;
    }
    if (pl.clusters.size() < 2u) {
        return "fewer than 2 clusters";
    }
    if (pl.clusters.size() > lim.max_clusters && !lim.multi_class) {
        return {refusal_code::too_many_clusters, "more than " + std::to_string(lim.max_clusters) + " clusters"};
    }

    // 2. Absorb single-source linear nodes into their source cluster.
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        const auto u = n_eq + i;
        if (!lim.absorb_linear || pl.cluster_of[u] != -1 || !is_glue_kind(p.nodes[i], cu)) {
            continue;
        }
        int src = -2;
        for (const auto &o : p.nodes[i].args) {
            if (!is_var(o)) {
                continue;
            }
            const auto c = o.idx < n_eq ? -1 : pl.cluster_of[o.idx];
            if (src == -2) {
                src = c;
            } else if (src != c) {
                src = -1;
            }
        }
        if (src >= 0) {
            pl.cluster_of[u] = src;
        }
    }
    for (std::uint32_t u = n_eq; u < n_u; ++u) {
        if (pl.cluster_of[u] >= 0) {
            pl.clusters[static_cast<std::size_t>(pl.cluster_of[u])].push_back(u);
        }
    }

    // Glue nodes must be of a kind evaluable from current-order values.
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        if (pl.cluster_of[n_eq + i] == -1 && !is_glue_kind(p.nodes[i], cu)) {
            return std::string("unsupported glue node kind: ") + func_kind_name(p.nodes[i].kind);
        }
    }

    // 3. Levels on the contracted graph. lvl of state variables = 0; a cluster runs as a unit.
    //    First pass: levels of glue nodes and provisional cluster levels, iterated to a fixed point
    //    (the graph is a DAG unless a cluster depends on itself through glue).
    const auto nc = pl.clusters.size();
    std::vector<std::uint32_t> clvl(nc, 1u);
    pl.lvl.assign(n_u, 0u);
    bool changed = true;
    std::uint32_t iters = 0;
    while (changed) {
        changed = false;
        if (++iters > n_u + 2u) {
            return "cyclic dependency between a cluster and glue nodes";
        }
        for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
            const auto u = n_eq + i;
            const auto c = pl.cluster_of[u];
            std::uint32_t need = 1;
            for (const auto &o : p.nodes[i].args) {
                if (!is_var(o)) {
                    continue;
                }
                const auto oc = o.idx < n_eq ? -1 : pl.cluster_of[o.idx];
                if (c >= 0 && oc == c) {
                    continue;
                }
                const auto ol = (oc >= 0) ? clvl[static_cast<std::size_t>(oc)] : pl.lvl[o.idx];
                need = std::max(need, ol + 1u);
            }
            if (c >= 0) {
                if (need > clvl[static_cast<std::size_t>(c)]) {
                    clvl[static_cast<std::size_t>(c)] = need;
                    changed = true;
                }
            } else if (need != pl.lvl[u]) {
                pl.lvl[u] = need;
                changed = true;
            }
        }
    }
    for (std::size_t c = 1; c < nc && !lim.multi_class; ++c) {
        if (clvl[c] != clvl[0]) {
            return "clusters at different dependency levels";
        }
    }
    pl.cluster_level = clvl[0];
    for (std::uint32_t u = n_eq; u < n_u; ++u) {
        if (pl.cluster_of[u] >= 0) {
            pl.lvl[u] = clvl[static_cast<std::size_t>(pl.cluster_of[u])];
        }
    }
    pl.max_level = *std::max_element(pl.lvl.begin(), pl.lvl.end());

    // 4. Which cluster members are read from outside their cluster (glue, other clusters, sv rules)?
    std::vector<char> exported(n_u, 0);
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        const auto c = pl.cluster_of[n_eq + i];
        for (const auto &o : p.nodes[i].args) {
            if (is_var(o) && o.idx >= n_eq && pl.cluster_of[o.idx] >= 0 && pl.cluster_of[o.idx] != c) {
                exported[o.idx] = 1;
            }
        }
    }
    for (const auto &d : p.sv_defs) {
        if (is_var(d) && d.idx >= n_eq && pl.cluster_of[d.idx] >= 0) {
            exported[d.idx] = 1;
        }
    }

    // 5. Isomorphism check + template-relative tables.
    const auto &t0 = pl.clusters[0];
    pl.ext_u.assign(nc, {});
    pl.cst_val.assign(nc, {});
    std::vector<std::string> sigs(nc);
    // Numerical operands that must be identical (they select the code shape).
    const auto structural_number = [](const dc_node &n, std::size_t a) {
        if (n.kind == func_kind::pow && a == 1u) {
            return true;
        }
        if (n.kind == func_kind::prod && a == 0u && n.args[0].type == operand::kind::num && n.args[0].value == -1.) {
            return true;
        }
        return false;
    };
    std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> num_pos(nc), par_pos(nc);
    std::vector<std::vector<double>> num_val(nc);
    std::vector<std::vector<std::uint32_t>> par_idx(nc);
    for (std::size_t c = 0; c < nc; ++c) {
        const auto &mem = pl.clusters[c];
        if (mem.size() != t0.size() && !lim.multi_class) {
            return {refusal_code::not_isomorphic, "clusters are not isomorphic (different sizes)"};
        }
        std::map<std::uint32_t, std::uint32_t> pos_of, ext_of;
        for (std::uint32_t q = 0; q < mem.size(); ++q) {
            pos_of[mem[q]] = q;
        }
        std::ostringstream sig;
        for (std::uint32_t q = 0; q < mem.size(); ++q) {
            const auto &n = p.nodes[mem[q] - n_eq];
            // NOTE: whether a member is read from outside is not part of the shape: a position is exported if it is in
            // any cluster (clusters padded by pad_clusters() carry members nobody reads).
            sig << func_kind_name(n.kind) << '(';
            for (std::size_t a = 0; a < n.args.size(); ++a) {
                const auto &o = n.args[a];
                if (is_var(o)) {
                    if (const auto it = pos_of.find(o.idx); it != pos_of.end()) {
                        sig << 'm' << it->second;
                    } else {
                        auto it2 = ext_of.find(o.idx);
                        if (it2 == ext_of.end()) {
                            it2 = ext_of.emplace(o.idx, static_cast<std::uint32_t>(pl.ext_u[c].size())).first;
                            pl.ext_u[c].push_back(o.idx);
                        }
                        sig << 'e' << it2->second;
                    }
                } else if (o.type == operand::kind::par) {
                    // Parameters: identical index across the clusters -> plain name, otherwise a per-lane table.
                    if (lim.generic_pars) {
                        sig << 'P';
                        par_pos[c].emplace_back(q, static_cast<std::uint32_t>(a));
                        par_idx[c].push_back(o.idx);
                    } else {
                        sig << 'p' << o.idx;
                    }
                } else if (n.kind == func_kind::pow && a == 1u) {
                    sig << 'n' << fp_literal(o.value);
                } else {
                    // NOTE: a factor -1 (a negation in the decomposition) is an ordinary constant here: -G m_i is -1 for a
                    // unit mass in G = 1 units and something else for the other bodies. Identical across the clusters ->
                    // it stays in the node (and the emitter negates); otherwise it becomes a per-lane constant and the
                    // emitter multiplies (ssa_emitter::node() checks for an override before taking the shortcut).
                    sig << 'c';
                    num_pos[c].emplace_back(q, static_cast<std::uint32_t>(a));
                    num_val[c].push_back(o.value);
                }
                sig << ',';
            }
            sig << ")[";
            for (const auto d : n.deps) {
                const auto it = pos_of.find(d);
                if (it == pos_of.end()) {
                    return "hidden dependency outside of its cluster";
                }
                sig << it->second << ',';
            }
            sig << ']';
        }
        sigs[c] = sig.str();
        if (sigs[c] != sigs[0] && !lim.multi_class) {
            return {refusal_code::not_isomorphic, "clusters are not isomorphic"};
        }
    }
    if (lim.multi_class) {
        return finish_multi_class_plan(p, order, pl, cu, clvl, sigs, num_pos, num_val, exported);
    }
    // Constants: literal if identical across clusters, otherwise a per-lane table entry.
    for (std::size_t j = 0; j < num_pos[0].size(); ++j) {
        bool same = true;
        for (std::size_t c = 1; c < nc; ++c) {
            const auto a = num_val[c][j], b = num_val[0][j];
            if (!(a == b || (std::isnan(a) && std::isnan(b))) || std::signbit(a) != std::signbit(b)) {
                same = false;
            }
        }
        if (!same) {
            pl.cst_pos.push_back(num_pos[0][j]);
            for (std::size_t c = 0; c < nc; ++c) {
                pl.cst_val[c].push_back(num_val[c][j]);
            }
        }
    }
    pl.par_idx.assign(nc, {});
    for (std::size_t j = 0; j < par_pos[0].size(); ++j) {
        bool same = true;
        for (std::size_t c = 1; c < nc; ++c) {
            same = same && par_idx[c][j] == par_idx[0][j];
        }
        if (!same) {
            pl.par_pos.push_back(par_pos[0][j]);
            for (std::size_t c = 0; c < nc; ++c) {
                pl.par_idx[c].push_back(par_idx[c][j]);
            }
        }
    }
    for (std::uint32_t q = 0; q < t0.size(); ++q) {
        bool any = false;
        for (std::size_t c = 0; c < nc; ++c) {
            any = any || exported[pl.clusters[c][q]] != 0;
        }
        if (any) {
            pl.out_pos.push_back(q);
        }
    }

    // 6. Lane-group width.
    pl.L = 2;
    while (pl.L < nc && pl.L < 64u) {
        pl.L *= 2u;
    }
    pl.spw = 64u / pl.L;

    // Register estimate: members whose history is needed keep `order` doubles alive.
    std::set<std::uint32_t> stored;
    for (const auto u : t0) {
        const auto &n = p.nodes[u - n_eq];
        for (const auto h : history_operands(n, cu)) {
            stored.insert(h);
        }
        switch (n.kind) {
            case func_kind::pow:
            case func_kind::div:
            case func_kind::sin:
            case func_kind::cos:
            case func_kind::exp:
            case func_kind::log:
            case func_kind::sigmoid:
            case func_kind::asin:
            case func_kind::acos:
            case func_kind::atan:
            case func_kind::asinh:
            case func_kind::acosh:
            case func_kind::atanh:
                if (!history_operands(n, cu).empty()) {
                    stored.insert(u);
                }
                break;
            default:
                break;
        }
    }
    if (lim.jets_in_registers && stored.size() * order * 2u > 420u) {
        return "the jets of a cluster do not fit in the register file";
    }
    for (std::uint32_t q = 0; q < t0.size(); ++q) {
        if (stored.count(t0[q]) != 0u) {
            pl.stored_pos.push_back(q);
        }
    }

    // 7. LDS slots: state variables, exported cluster members, glue nodes; then dummies.
    pl.slot_of.assign(n_u, -1);
    std::uint32_t ns = 0;
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        pl.slot_of[i] = static_cast<int>(ns++);
    }
    // NOTE: output-major numbering: the lanes of a group (one cluster each) write *consecutive* slots for a
    // given output, i.e. distinct LDS banks (cluster-major numbering gave a stride of n_out doubles between
    // lanes and 2-way bank conflicts on every ds_write_b64).
    for (const auto q : pl.out_pos) {
        for (std::size_t c = 0; c < nc; ++c) {
            pl.slot_of[pl.clusters[c][q]] = static_cast<int>(ns++);
        }
    }
    for (std::uint32_t u = n_eq; u < n_u; ++u) {
        if (pl.cluster_of[u] == -1) {
            pl.slot_of[u] = static_cast<int>(ns++);
        }
    }
    pl.n_slots = ns;

    // 8. Glue groups: per level, per shape.
    std::map<std::pair<std::uint32_t, std::string>, std::size_t> gidx;
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        const auto u = n_eq + i;
        if (pl.cluster_of[u] != -1) {
            continue;
        }
        const auto &n = p.nodes[i];
        std::ostringstream key;
        key << func_kind_name(n.kind);
        for (std::size_t a = 0; a < n.args.size(); ++a) {
            const auto &o = n.args[a];
            if (is_var(o)) {
                // (Constant factors of products are part of the shape: they select the linear rule.)
                key << ((cu != nullptr && n.kind == func_kind::prod && (*cu)[o.idx] != 0) ? "k" : "v");
            } else if (o.type == operand::kind::par) {
                // (Per-lane parameter tables in the pipelined generator; the first-generation one checks gpar_generic.)
                if (lim.generic_pars) {
                    key << "P";
                    pl.glue_has_par = true;
                } else {
                    key << "p" << o.idx;
                }
            } else if (structural_number(n, a)) {
                key << "n" << fp_literal(o.value);
            } else {
                key << "c";
            }
        }
        const auto k = std::make_pair(pl.lvl[u], key.str());
        auto it = gidx.find(k);
        if (it == gidx.end()) {
            it = gidx.emplace(k, pl.groups.size()).first;
            pl.groups.emplace_back();
            pl.groups.back().level = pl.lvl[u];
            pl.groups.back().key = key.str();
        }
        pl.groups[it->second].nodes.push_back(u);
    }
    std::stable_sort(pl.groups.begin(), pl.groups.end(),
                     [](const glue_group &a, const glue_group &b) { return a.level < b.level; });

    return {};
}

emit_refusal cluster_detail::make_plan(const taylor_program &p, std::uint32_t order, cluster_plan &pl,
                                       const plan_limits &lim)
{
    auto why = make_plan_impl(p, order, pl, lim);
    if (lim.absorb_linear && why.code == refusal_code::not_isomorphic) {
        // E.g. model::np1body with unit masses: the heliocentric clusters feed scaling products of their own, the pair
        // clusters do not. Without the absorption those products are glue and the clusters are isomorphic again.
        auto lim2 = lim;
        lim2.absorb_linear = false;
        cluster_plan pl2;
        const auto why2 = make_plan_impl(p, order, pl2, lim2);
        if (why2.empty()) {
            pl = std::move(pl2);
            return why2;
        }
    }
    return why;
}

} // namespace heyoka_amd
