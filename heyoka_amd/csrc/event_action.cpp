// Terminal-event actions. See event_action.hpp.
#include "event_action.hpp"

#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cfunc.hpp"
#include "hip_emit_detail.hpp"

namespace heyoka_amd
{

std::string event_action::to_string() const
{
    std::string ret = "event_action({";
    for (std::size_t i = 0; i < assignments.size(); ++i) {
        ret += (i != 0u ? ", " : "") + assignments[i].first.to_string() + ": " + assignments[i].second.to_string();
    }
    return ret + "})";
}

namespace detail
{

event_action_section make_event_action_section(const event_action &act, std::uint32_t te_idx,
                                               const std::vector<expression> &state_vars, std::uint32_t n_par)
{
    const auto where = " (terminal event " + std::to_string(te_idx) + ")";
    if (act.assignments.empty()) {
        throw std::invalid_argument("Cannot construct an event action from an empty list of assignments" + where);
    }
    const section_wording w{
        [&](std::size_t k, const std::string &v) {
            return "The right-hand side of the assignment to '" + act.assignments[k].first.to_string()
                   + "' in an event action uses the variable '" + v + "', which is not a state variable of the system" + where;
        },
        [&](std::uint32_t i, std::uint32_t n) {
            return "An event action uses par[" + std::to_string(i) + "], but the system and its event equations have "
                   + std::to_string(n) + " parameter(s)" + where;
        }};
    event_action_section ret;
    ret.te_idx = te_idx;
    ret.rows = assignment_rows(act.assignments, state_vars, w, "an event action", where);
    std::vector<expression> rhs;
    for (const auto &a : act.assignments) {
        rhs.push_back(a.second);
    }
    static_cast<expr_section &>(ret) = make_expr_section(rhs, state_vars, n_par, w);
    return ret;
}

std::string emit_assignment_section(const expr_section &sec, const std::vector<std::uint32_t> &rows)
{
    const auto &p = sec.prog;
    std::ostringstream src;
    const auto code = emit_order0(p, [](std::uint32_t i) { return "x" + std::to_string(i); });
    for (const auto r : sec.reads) {
        src << "const double x" << r << " = a.state[(u64)" << r << "u * N + s];\n";
    }
    for (std::uint32_t i = 0; i < p.n_par; ++i) {
        src << "const double par_" << i << " = a.pars[(u64)" << i << "u * N + s];\n";
    }
    if (p.time_dependent) {
        src << "const double t_hi = a.time_hi[s];\n";
    }
    src << code.body;
    // (Named results first: an output which is a plain copy of a row, or a literal, is a value of its own before any
    // row is written.)
    for (std::size_t o = 0; o < code.outs.size(); ++o) {
        src << "const double r" << o << " = " << code.outs[o] << ";\n";
    }
    for (std::size_t o = 0; o < rows.size(); ++o) {
        src << "a.state[(u64)" << rows[o] << "u * N + s] = r" << o << ";\n";
    }
    return src.str();
}

std::string make_event_action_source(const std::vector<event_action_section> &sections)
{
    std::ostringstream src;
    src << emit_detail::prelude();
    {
        // (The device code of the node rules of every section, once.)
        taylor_program all;
        for (const auto &sec : sections) {
            all.nodes.insert(all.nodes.end(), sec.prog.nodes.begin(), sec.prog.nodes.end());
        }
        src << emit_detail::rules_source(all);
    }
    src << "\n" << eva_kargs_text() << R"HIP(
// One lane per system. A system whose step ended at a terminal event with an action (continuing outcome = index of the
// event) runs the section of that event; every other system leaves after the load of its outcome. A section is
// straight-line code: the state rows it reads, parameters and time, all the right-hand sides, then the stores - every
// right-hand side sees the state from before the action.
extern "C" __global__ void __launch_bounds__(256) hy_ev_action(const hy_eva_args a)
{
    const u64 lane = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (lane >= a.count) return;
    const u64 s = a.first + lane;
    if (s >= N) return;
    const i64 oc = (a.force >= 0) ? a.force : a.outcome[s];
    switch (oc) {
)HIP";
    for (const auto &sec : sections) {
        src << "case " << sec.te_idx << ": {\n" << emit_assignment_section(sec, sec.rows);
        src << "break;\n}\n";
    }
    src << "default:\nbreak;\n}\n}\n";
    return src.str();
}

} // namespace detail

} // namespace heyoka_amd
