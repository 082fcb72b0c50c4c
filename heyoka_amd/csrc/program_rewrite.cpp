// The rewrites of the internal program: what each one is for is told in program_rewrite.hpp.
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <limits>
#include <map>
#include <numeric>
#include <set>

#include "hip_emit_cluster_plan.hpp"
#include "program_rewrite.hpp"

namespace heyoka_amd
{

namespace
{

using cluster_detail::history_operands;
using cluster_detail::is_var;

} // namespace

bool add_state_aliases(const taylor_program &p, taylor_program &out)
{
    const auto n_eq = p.n_eq;
    // Cluster members: nodes with history operands, and the u variables in history position.
    std::vector<char> member(p.n_u, 0);
    std::set<std::uint32_t> hist_sv;
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        const auto hs = history_operands(p.nodes[i]);
        if (!hs.empty()) {
            member[n_eq + i] = 1;
        }
        for (const auto h : hs) {
            if (h < n_eq) {
                hist_sv.insert(h);
            } else {
                member[h] = 1;
            }
        }
    }
    if (hist_sv.empty()) {
        return false;
    }
    // State variables read by members (in any position).
    std::set<std::uint32_t> used_sv(hist_sv.begin(), hist_sv.end());
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        if (member[n_eq + i] != 0) {
            for (const auto &o : p.nodes[i].args) {
                if (o.type == operand::kind::uvar && o.idx < n_eq) {
                    used_sv.insert(o.idx);
                }
            }
        }
    }

    out = p;
    out.nodes.clear();
    std::map<std::uint32_t, std::uint32_t> copy_of, alias_of;
    std::uint32_t next = n_eq;
    const auto uvar = [](std::uint32_t u) { return operand{operand::kind::uvar, u, 0.}; };
    for (const auto sv : used_sv) {
        dc_node g;
        g.kind = func_kind::sum;
        g.args.push_back(uvar(sv));
        out.nodes.push_back(g);
        copy_of[sv] = next++;
    }
    for (const auto sv : hist_sv) {
        dc_node z;
        z.kind = func_kind::num_identity;
        z.args.push_back(operand{operand::kind::num, 0u, 0.});
        out.nodes.push_back(z);
        dc_node a;
        a.kind = func_kind::sub;
        a.args.push_back(uvar(copy_of.at(sv)));
        a.args.push_back(uvar(next));
        out.nodes.push_back(a);
        alias_of[sv] = next + 1u;
        next += 2u;
    }
    const auto m = next - n_eq;
    const auto shift = [&](std::uint32_t u) { return u < n_eq ? u : u + m; };
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        auto nn = p.nodes[i];
        const auto hs = history_operands(p.nodes[i]);
        const bool is_member = member[n_eq + i] != 0;
        for (auto &o : nn.args) {
            if (o.type != operand::kind::uvar) {
                continue;
            }
            if (o.idx >= n_eq) {
                o.idx = shift(o.idx);
            } else if (std::find(hs.begin(), hs.end(), o.idx) != hs.end()) {
                o.idx = alias_of.at(o.idx);
            } else if (is_member) {
                o.idx = copy_of.at(o.idx);
            }
        }
        for (auto &d : nn.deps) {
            d = shift(d);
        }
        out.nodes.push_back(std::move(nn));
    }
    for (auto &d : out.sv_defs) {
        if (d.type == operand::kind::uvar) {
            d.idx = shift(d.idx);
        }
    }
    for (auto &e : out.ev_u) {
        e = shift(e);
    }
    out.n_u = p.n_u + m;
    return true;
}

bool insert_unit_scalings(const taylor_program &p, taylor_program &out)
{
    const auto n_eq = p.n_eq;
    constexpr auto none = std::numeric_limits<std::uint32_t>::max();
    std::vector<char> is_pow(p.n_u, 0), scaled(p.n_u, 0), direct(p.n_u, 0);
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        const auto &n = p.nodes[u - n_eq];
        is_pow[u] = (n.kind == func_kind::pow && n.args.size() == 2u && is_var(n.args[0])) ? 1 : 0;
    }
    for (const auto &n : p.nodes) {
        if (n.kind != func_kind::prod || n.args.size() != 2u) {
            continue;
        }
        for (std::size_t a = 0; a < 2u; ++a) {
            const auto &o = n.args[a], &other = n.args[1u - a];
            if (is_var(o) && is_pow[o.idx] != 0) {
                if (other.type == operand::kind::num || other.type == operand::kind::par) {
                    scaled[o.idx] = 1;
                } else if (is_var(other)) {
                    direct[o.idx] = 1;
                }
            }
        }
    }
    bool any_scaled = false, any_todo = false;
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        any_scaled = any_scaled || scaled[u] != 0;
        any_todo = any_todo || (direct[u] != 0 && scaled[u] == 0);
    }
    if (!any_scaled || !any_todo) {
        return false;
    }
    // New index of every old u variable: one slot is inserted behind each pow node to be scaled.
    std::vector<std::uint32_t> new_idx(p.n_u, none), scal_idx(p.n_u, none);
    std::uint32_t next = n_eq;
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        new_idx[i] = i;
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        new_idx[u] = next++;
        if (direct[u] != 0 && scaled[u] == 0) {
            scal_idx[u] = next++;
        }
    }
    out = p;
    out.nodes.clear();
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        auto nn = p.nodes[u - n_eq];
        const bool var_prod = nn.kind == func_kind::prod && nn.args.size() == 2u && is_var(nn.args[0]) && is_var(nn.args[1]);
        for (auto &o : nn.args) {
            if (o.type == operand::kind::uvar) {
                // (Only the products with a variable factor are rewired: other readers of the pow keep reading it.)
                o.idx = (var_prod && scal_idx[o.idx] != none) ? scal_idx[o.idx] : new_idx[o.idx];
            }
        }
        for (auto &d : nn.deps) {
            d = new_idx[d];
        }
        out.nodes.push_back(std::move(nn));
        if (scal_idx[u] != none) {
            dc_node sc;
            sc.kind = func_kind::prod;
            operand one;
            one.type = operand::kind::num;
            one.value = 1.;
            operand src;
            src.type = operand::kind::uvar;
            src.idx = new_idx[u];
            sc.args = {one, src};
            out.nodes.push_back(std::move(sc));
        }
    }
    for (auto &d : out.sv_defs) {
        if (d.type == operand::kind::uvar) {
            d.idx = new_idx[d.idx];
        }
    }
    for (auto &e : out.ev_u) {
        e = new_idx[e];
    }
    out.n_u = next;
    return true;
}

bool linearise_accelerations(const taylor_program &p, taylor_program &out)
{
    const auto n_eq = p.n_eq;
    constexpr auto none = std::numeric_limits<std::uint32_t>::max();
    if (!p.ev_u.empty() || p.n_par != 0u) {
        return false;
    }
    const auto node_of = [&](std::uint32_t u) -> const dc_node & { return p.nodes[u - n_eq]; };
    const auto is_num = [](const operand &o) { return o.type == operand::kind::num; };
    // Linear glue: sum over variables, sub of two variables, prod(number, variable).
    const auto linear = [&](std::uint32_t u) {
        if (u < n_eq) {
            return false;
        }
        const auto &n = node_of(u);
        if (!n.deps.empty()) {
            return false;
        }
        if (n.kind == func_kind::sum) {
            return !n.args.empty() && std::all_of(n.args.begin(), n.args.end(), [](const operand &o) { return is_var(o); });
        }
        if (n.kind == func_kind::sub) {
            return n.args.size() == 2u && is_var(n.args[0]) && is_var(n.args[1]);
        }
        return n.kind == func_kind::prod && n.args.size() == 2u && is_num(n.args[0]) && is_var(n.args[1]);
    };
    const auto leaf_ok = [&](std::uint32_t u) {
        if (u < n_eq) {
            return false;
        }
        const auto &n = node_of(u);
        return n.kind == func_kind::prod && n.args.size() == 2u && is_var(n.args[0]) && is_var(n.args[1]) && n.deps.empty();
    };
    // Flattened definitions.
    struct term {
        double c;
        std::uint32_t leaf;
    };
    std::vector<std::vector<term>> flat(n_eq);
    std::vector<char> removed(p.n_u, 0);
    bool ok = true, any_tree = false;
    const std::function<void(std::uint32_t, double, std::vector<term> &)> walk = [&](std::uint32_t u, double c, std::vector<term> &dst) {
        if (!ok) {
            return;
        }
        if (linear(u)) {
            removed[u] = 1;
            const auto &n = node_of(u);
            if (n.kind == func_kind::sum) {
                for (const auto &o : n.args) {
                    walk(o.idx, c, dst);
                }
            } else if (n.kind == func_kind::sub) {
                walk(n.args[0].idx, c, dst);
                walk(n.args[1].idx, -c, dst);
            } else {
                walk(n.args[1].idx, c * n.args[0].value, dst);
            }
            return;
        }
        if (!leaf_ok(u)) {
            ok = false;
            return;
        }
        dst.push_back({c, u});
    };
    std::vector<std::uint32_t> acc_vars;
    for (std::uint32_t i = 0; i < n_eq && ok; ++i) {
        const auto &d = p.sv_defs[i];
        if (d.type != operand::kind::uvar) {
            return false;
        }
        if (d.idx < n_eq) {
            continue; // (x' = v)
        }
        walk(d.idx, 1., flat[i]);
        acc_vars.push_back(i);
        const auto &root = node_of(d.idx);
        // (Already one sum over leaves and reactions: nothing to do for this variable.)
        any_tree = any_tree || !(root.kind == func_kind::sum && std::all_of(root.args.begin(), root.args.end(), [&](const operand &o) {
                                     return leaf_ok(o.idx);
                                 }));
    }
    if (!ok || acc_vars.size() < 2u || !any_tree) {
        return false;
    }
    const auto n_terms = flat[acc_vars[0]].size();
    if (n_terms < 2u) {
        return false;
    }
    // Appearances of every leaf: at most two, one of them with coefficient +1 (the direct product).
    std::map<std::uint32_t, std::vector<std::pair<std::uint32_t, double>>> app;
    for (const auto i : acc_vars) {
        if (flat[i].size() != n_terms) {
            return false;
        }
        for (const auto &t : flat[i]) {
            if (!std::isfinite(t.c) || t.c == 0.) {
                return false;
            }
            app[t.leaf].emplace_back(i, t.c);
        }
    }
    std::map<std::pair<std::uint32_t, std::uint32_t>, bool> is_reaction; // (variable, leaf) -> reads the reaction node
    std::map<std::uint32_t, double> rx_coef;                            // leaf -> coefficient of its reaction node
    for (const auto &[leaf, v] : app) {
        if (v.size() > 2u || (v.size() == 2u && v[0].first == v[1].first)) {
            return false;
        }
        std::size_t direct = v.size();
        for (std::size_t a = 0; a < v.size(); ++a) {
            if (v[a].second == 1.) {
                direct = a;
                break;
            }
        }
        if (direct == v.size()) {
            return false;
        }
        for (std::size_t a = 0; a < v.size(); ++a) {
            is_reaction[{v[a].first, leaf}] = a != direct;
            if (a != direct) {
                rx_coef[leaf] = v[a].second;
            }
        }
    }
    // The removed linear nodes must have no reader outside the trees.
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (removed[u] != 0) {
            continue;
        }
        for (const auto &o : node_of(u).args) {
            if (is_var(o) && removed[o.idx] != 0) {
                return false;
            }
        }
        for (const auto dd : node_of(u).deps) {
            if (removed[dd] != 0) {
                return false;
            }
        }
    }
    // New numbering: the kept nodes in their order, a reaction node right behind its product, the sums at the end.
    std::vector<std::uint32_t> new_idx(p.n_u, none), rx_idx(p.n_u, none);
    std::uint32_t next = n_eq;
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        new_idx[i] = i;
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (removed[u] != 0) {
            continue;
        }
        new_idx[u] = next++;
        if (rx_coef.count(u) != 0u) {
            rx_idx[u] = next++;
        }
    }
    out = p;
    out.nodes.clear();
    const auto uvar = [](std::uint32_t idx) {
        operand o;
        o.type = operand::kind::uvar;
        o.idx = idx;
        return o;
    };
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (removed[u] != 0) {
            continue;
        }
        auto nn = node_of(u);
        for (auto &o : nn.args) {
            if (o.type == operand::kind::uvar) {
                o.idx = new_idx[o.idx];
            }
        }
        for (auto &d : nn.deps) {
            d = new_idx[d];
        }
        out.nodes.push_back(std::move(nn));
        if (rx_idx[u] != none) {
            dc_node rx;
            rx.kind = func_kind::prod;
            operand c;
            c.type = operand::kind::num;
            c.value = rx_coef.at(u);
            rx.args = {c, uvar(new_idx[u])};
            out.nodes.push_back(std::move(rx));
        }
    }
    for (const auto i : acc_vars) {
        dc_node sm;
        sm.kind = func_kind::sum;
        for (const auto &t : flat[i]) {
            sm.args.push_back(uvar(is_reaction.at({i, t.leaf}) ? rx_idx[t.leaf] : new_idx[t.leaf]));
        }
        out.nodes.push_back(std::move(sm));
        out.sv_defs[i] = uvar(next++);
    }
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        if (p.sv_defs[i].idx < n_eq) {
            out.sv_defs[i] = p.sv_defs[i];
        }
    }
    out.n_u = next;
    return true;
}

bool externalise_scalings(const taylor_program &p, taylor_program &out)
{
    const auto n_eq = p.n_eq;
    constexpr auto none = std::numeric_limits<std::uint32_t>::max();
    if (!p.ev_u.empty() || p.n_par != 0u) {
        return false;
    }
    const auto node_of = [&](std::uint32_t u) -> const dc_node & { return p.nodes[u - n_eq]; };
    const auto is_num = [](const operand &o) { return o.type == operand::kind::num; };
    const auto scaled = [&](const dc_node &n) {
        return n.kind == func_kind::prod && n.args.size() == 2u && is_num(n.args[0]) && is_var(n.args[1]) && n.deps.empty();
    };
    const auto product = [&](const dc_node &n) {
        return n.kind == func_kind::prod && n.args.size() == 2u && is_var(n.args[0]) && is_var(n.args[1]) && n.deps.empty();
    };
    std::vector<std::vector<std::uint32_t>> readers(p.n_u);
    std::vector<char> dep_read(p.n_u, 0);
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        for (const auto &o : node_of(u).args) {
            if (is_var(o)) {
                readers[o.idx].push_back(u);
            }
        }
        for (const auto d : node_of(u).deps) {
            dep_read[d] = 1;
        }
    }
    std::vector<char> sv_read(p.n_u, 0);
    for (const auto &d : p.sv_defs) {
        if (d.type == operand::kind::uvar) {
            sv_read[d.idx] = 1;
        }
    }
    // Scaling nodes: number * pow, read by products only.
    std::map<std::uint32_t, std::pair<double, std::uint32_t>> scal;
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        const auto &n = node_of(u);
        if (!scaled(n) || n.args[1].idx < n_eq || node_of(n.args[1].idx).kind != func_kind::pow || dep_read[u] != 0 || sv_read[u] != 0
            || readers[u].empty()) {
            continue;
        }
        if (std::all_of(readers[u].begin(), readers[u].end(), [&](std::uint32_t r) {
                const auto &rn = node_of(r);
                return product(rn) && (rn.args[0].idx == u) != (rn.args[1].idx == u);
            })) {
            scal[u] = {n.args[0].value, n.args[1].idx};
        }
    }
    if (scal.empty()) {
        return false;
    }
    // The products which read them; their readers: sums / differences, or reactions number * product.
    std::map<std::uint32_t, double> scaled_prod;
    for (const auto &[s_u, cw] : scal) {
        for (const auto pr : readers[s_u]) {
            if (dep_read[pr] != 0) {
                return false;
            }
            for (const auto r : readers[pr]) {
                const auto &rn = node_of(r);
                const bool lin = rn.deps.empty() && (rn.kind == func_kind::sum || rn.kind == func_kind::sub || scaled(rn));
                if (!lin) {
                    return false;
                }
            }
            scaled_prod[pr] = cw.first;
        }
    }
    // New numbering: the scalings go, number * product right behind every product.
    std::vector<std::uint32_t> new_idx(p.n_u, none), a_idx(p.n_u, none);
    std::uint32_t next = n_eq;
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        new_idx[i] = i;
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (scal.count(u) != 0u) {
            continue;
        }
        new_idx[u] = next++;
        if (scaled_prod.count(u) != 0u) {
            a_idx[u] = next++;
        }
    }
    const auto uvar = [](std::uint32_t idx) {
        operand o;
        o.type = operand::kind::uvar;
        o.idx = idx;
        return o;
    };
    const auto num = [](double v) {
        operand o;
        o.type = operand::kind::num;
        o.value = v;
        return o;
    };
    // (What a reader of u reads now.)
    const auto reads = [&](std::uint32_t u) { return a_idx[u] != none ? a_idx[u] : new_idx[u]; };
    out = p;
    out.nodes.clear();
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (scal.count(u) != 0u) {
            continue;
        }
        auto nn = node_of(u);
        if (scaled_prod.count(u) != 0u) {
            for (auto &o : nn.args) {
                o.idx = (scal.count(o.idx) != 0u) ? new_idx[scal.at(o.idx).second] : reads(o.idx);
            }
            out.nodes.push_back(std::move(nn));
            dc_node a;
            a.kind = func_kind::prod;
            a.args = {num(scaled_prod.at(u)), uvar(new_idx[u])};
            out.nodes.push_back(std::move(a));
            continue;
        }
        if (scaled(nn) && scaled_prod.count(nn.args[1].idx) != 0u) {
            // Reaction: (c' c) * unit product.
            const auto pr = nn.args[1].idx;
            nn.args = {num(nn.args[0].value * scaled_prod.at(pr)), uvar(new_idx[pr])};
            out.nodes.push_back(std::move(nn));
            continue;
        }
        for (auto &o : nn.args) {
            if (o.type == operand::kind::uvar) {
                o.idx = reads(o.idx);
            }
        }
        for (auto &d : nn.deps) {
            d = new_idx[d];
        }
        out.nodes.push_back(std::move(nn));
    }
    for (auto &d : out.sv_defs) {
        if (d.type == operand::kind::uvar) {
            d.idx = reads(d.idx);
        }
    }
    out.n_u = next;
    return true;
}

namespace
{

bool node_of_is_pow(const taylor_program &p, std::uint32_t u)
{
    return u >= p.n_eq && p.nodes[u - p.n_eq].kind == func_kind::pow;
}

} // namespace

bool privatise_cluster_inputs(const taylor_program &p, taylor_program &out)
{
    const auto n_eq = p.n_eq;
    constexpr auto none = std::numeric_limits<std::uint32_t>::max();
    const auto node_of = [&](std::uint32_t u) -> const dc_node & { return p.nodes[u - n_eq]; };
    // Cheap linear members: sub(num, var), sub(var, num), prod(-1, var) over a STATE variable or u variable.
    const auto is_neg = [](const dc_node &n) {
        return n.kind == func_kind::prod && n.args.size() == 2u && n.args[0].type == operand::kind::num
               && n.args[0].value == -1. && is_var(n.args[1]);
    };
    const auto is_diff = [](const dc_node &n) {
        return n.kind == func_kind::sub && n.args.size() == 2u
               && ((n.args[0].type == operand::kind::num && is_var(n.args[1]))
                   || (is_var(n.args[0]) && n.args[1].type == operand::kind::num));
    };
    const auto cheap = [&](std::uint32_t u) { return u >= n_eq && (is_neg(node_of(u)) || is_diff(node_of(u))); };

    // The heads: sums of squares over cheap members only.
    std::vector<std::uint32_t> heads;
    std::vector<std::uint32_t> n_head_readers(p.n_u, 0u);
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        const auto &n = node_of(u);
        if (n.kind != func_kind::sum_sq || n.args.empty()) {
            continue;
        }
        bool ok = true;
        for (const auto &o : n.args) {
            ok = ok && is_var(o) && cheap(o.idx);
        }
        if (ok) {
            heads.push_back(u);
            for (const auto &o : n.args) {
                ++n_head_readers[o.idx];
            }
        }
    }
    if (heads.size() < 2u) {
        return false;
    }
    bool needed = false;
    bool any_diff = false;
    for (const auto h : heads) {
        for (const auto &o : node_of(h).args) {
            needed = needed || n_head_readers[o.idx] > 1u || is_neg(node_of(o.idx));
            any_diff = any_diff || is_diff(node_of(o.idx));
        }
    }
    if (!needed || !any_diff) {
        return false;
    }
    // Which head does a u variable hang off? pow(head, c) and the scalings num * pow / par * pow of it.
    std::vector<std::uint32_t> head_of(p.n_u, none);
    for (const auto h : heads) {
        head_of[h] = h;
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        const auto &n = node_of(u);
        if (n.kind == func_kind::pow && n.args.size() == 2u && is_var(n.args[0]) && head_of[n.args[0].idx] != none) {
            head_of[u] = head_of[n.args[0].idx];
        } else if (n.kind == func_kind::prod && n.args.size() == 2u && !is_var(n.args[0]) && is_var(n.args[1])
                   && node_of_is_pow(p, n.args[1].idx) && head_of[n.args[1].idx] != none) {
            head_of[u] = head_of[n.args[1].idx];
        }
    }
    // Private copies: copy_idx[(head, position)] in the new numbering; readers: the head itself and the products
    // cheap * (pow chain of the head).
    struct rewire {
        std::uint32_t node, arg, head, pos;
    };
    std::vector<rewire> rw;
    std::vector<std::uint32_t> other_readers(p.n_u, 0u);
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        const auto &n = node_of(u);
        if (head_of[u] == u) {
            continue; // (a head: handled below)
        }
        for (std::size_t a = 0; a < n.args.size(); ++a) {
            const auto &o = n.args[a];
            if (!is_var(o) || !cheap(o.idx) || n_head_readers[o.idx] == 0u) {
                continue;
            }
            bool done = false;
            if (n.kind == func_kind::prod && n.args.size() == 2u && is_var(n.args[1u - a])) {
                const auto h = head_of[n.args[1u - a].idx];
                if (h != none) {
                    const auto &ha = node_of(h).args;
                    for (std::uint32_t q = 0; q < ha.size(); ++q) {
                        if (ha[q].idx == o.idx) {
                            rw.push_back({u, static_cast<std::uint32_t>(a), h, q});
                            done = true;
                            break;
                        }
                    }
                }
            }
            if (!done) {
                ++other_readers[o.idx];
            }
        }
    }
    for (const auto &d : p.sv_defs) {
        if (d.type == operand::kind::uvar && d.idx < p.n_u) {
            ++other_readers[d.idx];
        }
    }
    for (const auto e : p.ev_u) {
        ++other_readers[e];
    }
    // New numbering: the originals which keep a reader stay where they are, the copies of a head go right in front of it.
    std::vector<std::uint32_t> new_idx(p.n_u, none);
    std::map<std::pair<std::uint32_t, std::uint32_t>, std::uint32_t> copy_idx;
    std::uint32_t next = n_eq;
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        new_idx[i] = i;
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (cheap(u) && n_head_readers[u] != 0u && other_readers[u] == 0u) {
            continue; // dropped
        }
        if (head_of[u] == u) {
            for (std::uint32_t q = 0; q < node_of(u).args.size(); ++q) {
                copy_idx[{u, q}] = next++;
            }
        }
        new_idx[u] = next++;
    }
    out = p;
    out.nodes.clear();
    std::map<std::pair<std::uint32_t, std::uint32_t>, std::pair<std::uint32_t, std::uint32_t>> rw_of;
    for (const auto &r : rw) {
        rw_of[{r.node, r.arg}] = {r.head, r.pos};
    }
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        if (new_idx[u] == none) {
            continue;
        }
        auto nn = node_of(u);
        if (head_of[u] == u) {
            for (std::uint32_t q = 0; q < nn.args.size(); ++q) {
                auto c = node_of(nn.args[q].idx);
                if (is_neg(c)) {
                    // -1 * x -> -0.0 - x.
                    const auto var = c.args[1];
                    c.kind = func_kind::sub;
                    c.args[0].type = operand::kind::num;
                    c.args[0].value = -0.;
                    c.args[1] = var;
                }
                for (auto &o : c.args) {
                    if (o.type == operand::kind::uvar) {
                        o.idx = new_idx[o.idx];
                    }
                }
                out.nodes.push_back(std::move(c));
                nn.args[q].idx = copy_idx[{u, q}];
            }
        } else {
            for (std::size_t a = 0; a < nn.args.size(); ++a) {
                auto &o = nn.args[a];
                if (o.type != operand::kind::uvar) {
                    continue;
                }
                const auto it = rw_of.find({u, static_cast<std::uint32_t>(a)});
                o.idx = (it != rw_of.end()) ? copy_idx[it->second] : new_idx[o.idx];
            }
        }
        for (auto &d : nn.deps) {
            d = new_idx[d];
        }
        out.nodes.push_back(std::move(nn));
    }
    for (auto &d : out.sv_defs) {
        if (d.type == operand::kind::uvar) {
            d.idx = new_idx[d.idx];
        }
    }
    for (auto &e : out.ev_u) {
        e = new_idx[e];
    }
    out.n_u = next;
    return true;
}

bool pad_clusters(const taylor_program &p, std::uint32_t order, taylor_program &out)
{
    using cluster_detail::cluster_plan;
    cluster_plan pl;
    const auto why = cluster_detail::make_plan_impl(p, order, pl, cluster_detail::plan_limits{});
    if (why.code != refusal_code::not_isomorphic || pl.clusters.size() < 2u) {
        return false;
    }
    const auto n_eq = p.n_eq;
    const auto nc = pl.clusters.size();
    std::size_t tmax = 0;
    for (std::size_t c = 1; c < nc; ++c) {
        if (pl.clusters[c].size() > pl.clusters[tmax].size()) {
            tmax = c;
        }
    }
    const auto &T = pl.clusters[tmax];
    std::map<std::uint32_t, std::uint32_t> tpos;
    for (std::uint32_t q = 0; q < T.size(); ++q) {
        tpos[T[q]] = q;
    }
    // (Like the cluster signatures of make_plan(): a factor -1 is an ordinary per-cluster constant.)
    const auto structural_number = [](const dc_node &n, std::size_t a) { return n.kind == func_kind::pow && a == 1u; };
    constexpr auto none = std::numeric_limits<std::uint32_t>::max();

    // New members get provisional indices p.n_u, p.n_u + 1, ... and an anchor: the (old) u variable after which they are
    // inserted, so that the members of a padded cluster come in the order of the template (the planner compares the
    // clusters member by member, in ascending order of their indices).
    std::vector<dc_node> new_nodes;
    std::vector<std::uint32_t> anchor_of; // per new node: old u variable it follows (none: before the first node)
    std::uint32_t next_u = p.n_u;
    bool padded_any = false;
    for (std::size_t c = 0; c < nc; ++c) {
        if (c == tmax) {
            continue;
        }
        const auto &S = pl.clusters[c];
        std::map<std::uint32_t, std::uint32_t> spos;
        for (std::uint32_t q = 0; q < S.size(); ++q) {
            spos[S[q]] = q;
        }
        std::vector<std::uint32_t> f(S.size(), none);      // S position -> T position
        std::vector<char> used(T.size(), 0);
        std::map<std::uint32_t, std::uint32_t> ext_t2s, ext_s2t; // external inputs: T's u <-> S's u
        std::uint64_t budget = 200000;
        // Try to map S[i], S[i+1], ... (ascending u: the arguments of a member precede it).
        std::function<bool(std::size_t)> rec = [&](std::size_t i) -> bool {
            if (i == S.size()) {
                return true;
            }
            if (budget-- == 0u) {
                return false;
            }
            const auto &ns = p.nodes[S[i] - n_eq];
            for (std::uint32_t q = 0; q < T.size(); ++q) {
                const auto &nt = p.nodes[T[q] - n_eq];
                if (used[q] != 0 || nt.kind != ns.kind || nt.args.size() != ns.args.size() || nt.deps.size() != ns.deps.size()) {
                    continue;
                }
                bool ok = true;
                std::vector<std::pair<std::uint32_t, std::uint32_t>> added; // tentative external pairs (T u, S u)
                for (std::size_t a = 0; ok && a < ns.args.size(); ++a) {
                    const auto &so = ns.args[a], &to = nt.args[a];
                    if (so.type != to.type) {
                        ok = false;
                    } else if (is_var(so)) {
                        const auto it_t = tpos.find(to.idx);
                        const auto it_s = spos.find(so.idx);
                        if ((it_t == tpos.end()) != (it_s == spos.end())) {
                            ok = false;
                        } else if (it_t != tpos.end()) {
                            ok = f[it_s->second] == it_t->second;
                        } else {
                            const auto e1 = ext_t2s.find(to.idx);
                            const auto e2 = ext_s2t.find(so.idx);
                            if (e1 != ext_t2s.end() || e2 != ext_s2t.end()) {
                                ok = e1 != ext_t2s.end() && e2 != ext_s2t.end() && e1->second == so.idx && e2->second == to.idx;
                            } else {
                                ext_t2s[to.idx] = so.idx;
                                ext_s2t[so.idx] = to.idx;
                                added.emplace_back(to.idx, so.idx);
                            }
                        }
                    } else if (so.type == operand::kind::num) {
                        if (structural_number(nt, a) || structural_number(ns, a)) {
                            ok = so.value == to.value;
                        }
                    }
                }
                for (std::size_t d = 0; ok && d < ns.deps.size(); ++d) {
                    const auto it_t = tpos.find(nt.deps[d]);
                    const auto it_s = spos.find(ns.deps[d]);
                    ok = it_t != tpos.end() && it_s != spos.end() && f[it_s->second] == it_t->second;
                }
                if (ok) {
                    f[i] = q;
                    used[q] = 1;
                    if (rec(i + 1u)) {
                        return true;
                    }
                    used[q] = 0;
                    f[i] = none;
                }
                for (const auto &[tu, su] : added) {
                    ext_t2s.erase(tu);
                    ext_s2t.erase(su);
                }
            }
            return false;
        };
        if (!rec(0)) {
            return false;
        }
        // Members of the template the cluster lacks: appended to the program, in template order.
        std::vector<std::uint32_t> inv(T.size(), none); // T position -> u variable of this cluster
        for (std::size_t i = 0; i < S.size(); ++i) {
            inv[f[i]] = S[i];
        }
        std::uint32_t fallback_ext = none;
        for (const auto &[su, tu] : ext_s2t) {
            (void)tu;
            fallback_ext = su;
            break;
        }
        for (std::uint32_t q = 0; q < T.size(); ++q) {
            if (inv[q] != none) {
                continue;
            }
            auto nn = p.nodes[T[q] - n_eq];
            for (auto &o : nn.args) {
                if (o.type != operand::kind::uvar) {
                    continue;
                }
                if (const auto it = tpos.find(o.idx); it != tpos.end()) {
                    if (inv[it->second] == none) {
                        return false; // (template order is topological: cannot happen)
                    }
                    o.idx = inv[it->second];
                } else if (const auto e = ext_t2s.find(o.idx); e != ext_t2s.end()) {
                    o.idx = e->second;
                } else if (fallback_ext != none) {
                    o.idx = fallback_ext;
                } else {
                    return false;
                }
            }
            for (auto &d : nn.deps) {
                const auto it = tpos.find(d);
                if (it == tpos.end() || inv[it->second] == none) {
                    return false;
                }
                d = inv[it->second];
            }
            // Anchor: the member at the previous template position (or its anchor, if that one is new as well).
            std::uint32_t anc = none;
            if (q > 0u) {
                const auto prev = inv[q - 1u];
                anc = prev < p.n_u ? prev : anchor_of[prev - p.n_u];
            } else if (!S.empty() && S[0] > n_eq) {
                anc = S[0] - 1u;
            }
            new_nodes.push_back(std::move(nn));
            anchor_of.push_back(anc);
            inv[q] = next_u++;
            padded_any = true;
        }
    }
    if (!padded_any) {
        return false;
    }
    // Rebuild the program with the new members at their places; remap every u-variable index.
    std::vector<std::uint32_t> new_idx(next_u, none);
    std::vector<const dc_node *> order_nodes;
    std::vector<std::uint32_t> order_old; // provisional / old index of the nodes in the new order
    const auto place_after = [&](std::uint32_t anc) {
        for (std::size_t j = 0; j < new_nodes.size(); ++j) {
            if (anchor_of[j] == anc) {
                order_nodes.push_back(&new_nodes[j]);
                order_old.push_back(p.n_u + static_cast<std::uint32_t>(j));
            }
        }
    };
    place_after(none);
    for (std::uint32_t u = n_eq; u < p.n_u; ++u) {
        order_nodes.push_back(&p.nodes[u - n_eq]);
        order_old.push_back(u);
        place_after(u);
    }
    // NOTE: members anchored at a state variable (a cluster whose first member directly follows the state) land first.
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        new_idx[i] = i;
    }
    for (std::size_t j = 0; j < order_old.size(); ++j) {
        new_idx[order_old[j]] = n_eq + static_cast<std::uint32_t>(j);
    }
    for (std::size_t j = 0; j < new_nodes.size(); ++j) {
        if (new_idx[p.n_u + j] == none) {
            return false; // anchored at something which is not a node (cannot happen for anchors >= n_eq)
        }
    }
    out = p;
    out.nodes.clear();
    for (const auto *np : order_nodes) {
        auto nn = *np;
        for (auto &o : nn.args) {
            if (o.type == operand::kind::uvar) {
                o.idx = new_idx[o.idx];
            }
        }
        for (auto &d : nn.deps) {
            d = new_idx[d];
        }
        out.nodes.push_back(std::move(nn));
    }
    for (auto &d : out.sv_defs) {
        if (d.type == operand::kind::uvar) {
            d.idx = new_idx[d.idx];
        }
    }
    for (auto &e : out.ev_u) {
        e = new_idx[e];
    }
    out.n_u = next_u;
    // Arguments must precede their users.
    for (std::size_t j = 0; j < out.nodes.size(); ++j) {
        for (const auto &o : out.nodes[j].args) {
            if (o.type == operand::kind::uvar && o.idx >= n_eq + j) {
                return false;
            }
        }
    }
    return true;
}

} // namespace heyoka_amd
