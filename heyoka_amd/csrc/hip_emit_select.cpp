// emit_hip_module(): which stepper a program gets. emit_mode::cluster is a ladder of attempts (DESIGN 4.1 lists the rungs): the
// wave-cluster kernels on the decomposition, then on rewritten INTERNAL programs (program_rewrite.hpp), block mode, the multi-class
// plan, the generic steppers. A rung reacts to the refusal_code of an earlier attempt, never to the wording of a diagnostic.
#include "hip_emit_detail.hpp"
#include "program_rewrite.hpp"
#include "taylor_adaptive_batch.hpp"

#include <cstdio>

namespace heyoka_amd
{

std::string program_to_string(const taylor_program &p)
{
    std::ostringstream oss;
    const auto op = [&](const operand &o) {
        char buf[64];
        switch (o.type) {
            case operand::kind::uvar:
                oss << "u_" << o.idx;
                break;
            case operand::kind::num:
                std::snprintf(buf, sizeof(buf), "%.17g", o.value);
                oss << buf;
                break;
            default:
                oss << "p" << o.idx;
        }
    };
    for (const auto &n : p.nodes) {
        oss << func_kind_name(n.kind) << '(';
        for (std::size_t a = 0; a < n.args.size(); ++a) {
            if (a != 0u) {
                oss << ", ";
            }
            op(n.args[a]);
        }
        oss << ')';
        for (const auto d : n.deps) {
            oss << " [dep " << d << "]";
        }
        oss << '\n';
    }
    for (const auto &d : p.sv_defs) {
        op(d);
        oss << '\n';
    }
    return oss.str();
}

namespace
{

using enum refusal_code;

// What the rungs share. A rung returns true when its module m serves the program.
struct ladder {
    const taylor_program &prog;
    const emit_options &opts;
    emitted_module first;             // the wave-cluster kernels on the decomposition as it is
    emit_refusal why;                 // code: why `first` was refused, for good; text: that diagnostic, then those of the retries
    bool seen_not_isomorphic = false; // `first`, or a retry so far, was refused as not isomorphic
    bool refused(std::string &to, const char *what, const emit_refusal &r)
    {
        to += what + r.text;
        seen_not_isomorphic = seen_not_isomorphic || r.code == not_isomorphic;
        return false;
    }
};

// The code generated from a rewritten program serves the system: the note of the rewrite, the text of the program.
bool won(emitted_module &m, const std::string &note, const taylor_program &internal)
{
    m.notes += note;
    m.internal_program = program_to_string(internal);
    return true;
}

// The wave-cluster kernels on p; not isomorphic: on p with padded clusters. Returns the program of the last attempt (p, `padded`).
const taylor_program &emit_or_pad(const taylor_program &p, const emit_options &opts, taylor_program &padded, emitted_module &m, emit_refusal &why)
{
    m = emit_cluster_or_empty(p, opts, why);
    if (m.source.empty() && why.code == not_isomorphic && pad_clusters(p, opts.order, padded)) {
        m = emit_cluster_or_empty(padded, opts, why);
        return padded;
    }
    return p;
}

// Too many clusters for one wavefront: the same program in block mode (one system per workgroup). Returns block mode's refusal.
emit_refusal or_block(const taylor_program &p, const emit_options &opts, emitted_module &m, const emit_refusal &why)
{
    emit_refusal why_b;
    if (m.source.empty() && why.code == too_many_clusters) {
        m = emit_block(p, opts, why_b);
    }
    return why_b;
}

// 1. Accelerations which are not plain sums over the partners (equal or repeated masses) miss the one-lane-per-pair kernel only
// because of that: retry with the accelerations flattened (linearise_accelerations()). Taken when it gives a better kernel
// (emitted_module::cluster_generation: 5 one lane per pair > 3 lane pairs > 2 pipelined > 1 first generation).
bool linearised(const ladder &s, emitted_module &m)
{
    const auto kernel_rank = [](const emitted_module &em) { return em.source.empty() ? 0 : em.cluster_generation; };
    taylor_program lin, lin_scaled;
    if (!s.opts.dev.linearise || s.opts.dev.cluster_v1 || s.opts.cluster_kernel == 1 || kernel_rank(s.first) >= 5 || !linearise_accelerations(s.prog, lin)) {
        return false;
    }
    emit_refusal why;
    m = emit_cluster_or_empty(lin, s.opts, why);
    if (m.source.empty() && why.code == not_isomorphic && insert_unit_scalings(lin, lin_scaled)) {
        m = emit_cluster_or_empty(lin_scaled, s.opts, why);
        lin = std::move(lin_scaled);
    }
    return kernel_rank(m) > kernel_rank(s.first)
           && won(m, "; accelerations rewritten as flat sums of scaled pair products in the internal program "
                     "(re-associated additions: equal to the decomposition to rounding)", lin);
}

// 2. (and inside 7.) `why` is state_var_history: add_state_aliases(), then the single-class kernels and block mode, or the multi-class plan.
bool with_state_aliases(ladder &s, bool multi, emit_refusal &why, emitted_module &m)
{
    taylor_program aliased;
    emit_refusal why2;
    if (why.code != state_var_history || !s.opts.dev.state_aliases || !add_state_aliases(s.prog, aliased)) {
        return false;
    }
    m = multi ? emit_cluster_multi_or_empty(aliased, s.opts, why2) : emit_cluster_or_empty(aliased, s.opts, why2);
    if (!multi) {
        or_block(aliased, s.opts, m, why2);
    }
    return m.source.empty() ? s.refused(why.text, "; with state-variable aliases: ", why2)
                            : won(m, "; state variables in history-operand position aliased by u variables", aliased);
}

// 3. not_isomorphic: clusters which are sub-shapes of the largest one (test particles next to massive bodies), pad_clusters().
bool padded_clusters(ladder &s, emitted_module &m)
{
    taylor_program padded;
    emit_refusal why2;
    if (!pad_clusters(s.prog, s.opts.order, padded)) {
        return false;
    }
    m = emit_cluster_or_empty(padded, s.opts, why2);
    return m.source.empty() ? s.refused(s.why.text, "; with padded clusters: ", why2)
                            : won(m, "; clusters of " + std::to_string(padded.n_u - s.prog.n_u) + " missing members padded to the shape of the largest one", padded);
}

// 4. not_isomorphic: clusters which differ by an elided unit factor (unit masses next to others), insert_unit_scalings(), then padding.
bool unit_scalings(ladder &s, emitted_module &m)
{
    taylor_program scaled, padded;
    emit_refusal why3;
    if (!insert_unit_scalings(s.prog, scaled)) {
        return false;
    }
    const auto &base = emit_or_pad(scaled, s.opts, padded, m, why3);
    return m.source.empty() ? s.refused(s.why.text, "; with unit scalings: ", why3)
                            : won(m, "; " + std::to_string(base.n_u - s.prog.n_u) + " members added to the internal program (unit scalings of elided factors, padding)", base);
}

// 5. not_isomorphic, in the first attempt or in a retry: clusters which share coordinate differences (fixed centres / mascons),
// privatise_cluster_inputs(); then the unit scalings and the padding on top of it; wave-cluster kernels, or block mode.
bool private_inputs(ladder &s, emitted_module &m)
{
    std::vector<taylor_program> variants(2);
    if (!privatise_cluster_inputs(s.prog, variants[0])) {
        return false;
    }
    if (!insert_unit_scalings(variants[0], variants[1])) {
        variants.pop_back();
    }
    std::string why_p; // (The notes keep the refusal of the last variant.)
    for (const auto &v : variants) {
        emit_refusal why;
        taylor_program padded;
        const auto &base = emit_or_pad(v, s.opts, padded, m, why);
        const auto why_b = or_block(base, s.opts, m, why);
        const auto added = static_cast<long long>(base.n_u) - static_cast<long long>(s.prog.n_u);
        if (!m.source.empty()) {
            return won(m, "; internal program with private coordinate differences per cluster (" + std::to_string(added) + " members more than the decomposition)", base);
        }
        why_p = why.text + (why_b.empty() ? "" : ("; block mode: " + why_b.text));
    }
    s.why.text += "; with private cluster inputs: " + why_p;
    return false;
}

// 6. too_many_clusters: one system per workgroup, used whenever it is applicable (5x ... 44x the table steppers: DESIGN 4.1).
bool block_mode(ladder &s, emitted_module &m)
{
    emit_refusal why_b, why_e;
    m = emit_block(s.prog, s.opts, why_b);
    // (Distinct masses: scalings inside the clusters keep the decomposition off the v2 cluster phase, see externalise_scalings().)
    taylor_program ext;
    if (s.opts.dev.linearise && !m.block_v2_phase && !s.opts.exact_division && externalise_scalings(s.prog, ext)) {
        auto o2 = s.opts;
        o2.block_no_absorb = true;
        auto m2 = emit_block(ext, o2, why_e);
        if (!m2.source.empty() && m2.block_v2_phase) {
            m = std::move(m2);
            return won(m, "; scalings of the pair products moved out of the clusters in the internal program (c (d r^-3) for d (c r^-3): equal to the decomposition to rounding)", ext);
        }
    }
    if (!m.source.empty()) {
        return true;
    }
    s.why.text += why_b.empty() ? "; block mode: too few clusters" : ("; block mode: " + why_b.text);
    return why_b.code == not_isomorphic && private_inputs(s, m);
}

// 7. Clusters of several shapes or at several dependency levels: one section of straight-line code per CLASS of clusters
// (emit_cluster_v1() on a multi-class plan). Decompositions small enough for straight-line code on ONE lane stay there.
bool multi_class(ladder &s, emitted_module &m)
{
    if (!s.opts.dev.multi_class || s.opts.event_stepper || s.prog.nodes.size() <= s.opts.unroll_max_nodes) {
        return false;
    }
    emit_refusal why_m;
    m = emit_cluster_multi_or_empty(s.prog, s.opts, why_m);
    if (m.source.empty() && !with_state_aliases(s, true, why_m, m)) {
        s.why.text += "; multi-class plan: " + why_m.text;
        return false;
    }
    m.notes += " (single-class planners: " + s.why.text + ")";
    return true;
}

emitted_module select_cluster_stepper(const taylor_program &prog, const emit_options &opts)
{
    ladder s{prog, opts, {}, {}, false};
    s.first = emit_cluster_or_empty(prog, opts, s.why);
    s.seen_not_isomorphic = s.why.code == not_isomorphic;
    emitted_module m;
    if (linearised(s, m)) {
        return m;
    }
    if (!s.first.source.empty()) {
        return std::move(s.first);
    }
    if (with_state_aliases(s, false, s.why, m) || (s.why.code == not_isomorphic && (padded_clusters(s, m) || unit_scalings(s, m)))
        || (s.seen_not_isomorphic && private_inputs(s, m)) || (s.why.code == too_many_clusters && block_mode(s, m)) || multi_class(s, m)) {
        return m;
    }
    // 8. Not applicable to this DAG: the generic one-system-per-lane code, unrolled for small decompositions, else table-driven.
    auto u = (prog.nodes.size() > opts.unroll_max_nodes) ? emit_table(prog, opts) : emit_detail::emit_unrolled(prog, opts);
    u.notes += (u.notes.empty() ? "" : "; ") + ("cluster mode not applicable: " + s.why.text);
    u.cluster_fallback = true;
    return u;
}

} // namespace

emitted_module emit_hip_module(const taylor_program &prog, const emit_options &opts)
{
    if (opts.order < 2u) {
        throw std::invalid_argument("The Taylor order must be at least 2");
    }
    emit_refusal why;
    switch (opts.mode) {
        case emit_mode::unrolled:
            return emit_detail::emit_unrolled(prog, opts);
        case emit_mode::cluster:
            return select_cluster_stepper(prog, opts);
        case emit_mode::table:
            return emit_table(prog, opts);
        case emit_mode::block:
            if (auto b = emit_block(prog, opts, why); !b.source.empty()) {
                return b;
            }
            throw std::invalid_argument("Block mode is not applicable to this system: " + why.text);
        default:
            throw not_implemented_error("The requested code generation mode is not implemented yet");
    }
}

} // namespace heyoka_amd
