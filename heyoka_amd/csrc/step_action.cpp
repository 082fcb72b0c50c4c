// step_action. See step_action.hpp.
#include "step_action.hpp"

#include <ostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "angle_reducer.hpp"
#include "event_action.hpp"
#include "hip_emit_detail.hpp"

namespace heyoka_amd
{

step_action::step_action(std::vector<std::pair<expression, expression>> assignments, std::optional<expression> stop_when)
    : m_assignments(std::move(assignments)), m_stop_when(std::move(stop_when))
{
    if (m_assignments.empty() && !m_stop_when) {
        throw std::invalid_argument("Cannot construct a step action with neither assignments nor a stop condition");
    }
    for (const auto &[lhs, ex] : m_assignments) {
        (void)ex;
        if (!lhs.is_variable()) {
            throw std::invalid_argument("The left-hand side '" + lhs.to_string()
                                        + "' of an assignment of a step action is not a variable");
        }
    }
}

step_action::step_action(expression stop_when) : step_action({}, std::optional<expression>(std::move(stop_when))) {}

std::string step_action::to_string() const
{
    std::string ret = "step_action({";
    for (std::size_t i = 0; i < m_assignments.size(); ++i) {
        ret += (i != 0u ? ", " : "") + m_assignments[i].first.to_string() + ": " + m_assignments[i].second.to_string();
    }
    ret += "}";
    if (m_stop_when) {
        ret += ", stop_when=" + m_stop_when->to_string();
    }
    return ret + ")";
}

std::ostream &operator<<(std::ostream &os, const step_action &a)
{
    return os << a.to_string();
}

bool step_action::operator()(detail::tab_core &core)
{
    return core.apply_step_action(*this);
}

bool step_action::operator()(taylor_adaptive_batch<double> &ta)
{
    return ta.core().apply_step_action(*this);
}

namespace detail
{

step_action_section make_step_action_section(const step_action &act, const std::vector<expression> &state_vars,
                                             std::uint32_t n_par)
{
    const auto &asg = act.get_assignments();
    const section_wording w{
        [&](std::size_t k, const std::string &v) {
            return (k < asg.size() ? "The right-hand side of the assignment to '" + asg[k].first.to_string() + "'"
                                   : std::string("The stop condition"))
                   + " of a step action uses the variable '" + v + "', which is not a state variable of the system";
        },
        [](std::uint32_t i, std::uint32_t n) {
            return "A step action uses par[" + std::to_string(i) + "], but the integrator has " + std::to_string(n) + " parameter(s)";
        }};
    step_action_section ret;
    ret.rows = assignment_rows(asg, state_vars, w, "a step action");
    std::vector<expression> fn;
    for (const auto &a : asg) {
        fn.push_back(a.second);
    }
    if (act.get_stop_when()) {
        fn.push_back(*act.get_stop_when());
        ret.has_cond = true;
    }
    static_cast<expr_section &>(ret) = make_expr_section(fn, state_vars, n_par, w);
    return ret;
}

std::string make_step_action_source(const step_action_section &sec)
{
    const auto &p = sec.prog;
    std::ostringstream src;
    src << emit_detail::prelude() << emit_detail::rules_source(p);
    src << "\n" << emit_detail::outcome_define("HY_SA_CB_STOP", taylor_outcome::cb_stop) << "\n" << sa_kargs_text() << R"HIP(
// One lane per system. A system whose last step had zero length (it has reached its final time, or was retired) leaves
// after the load of last_h. The section is straight-line code: the state rows it reads, parameters and time, all the
// right-hand sides and the condition, then the stores - every expression sees the state from before the action. Stop
// flag: the lanes of a wavefront are combined with a ballot, the lowest of them adds their number to the counter. Under
// the independent semantics (retired != nullptr) the stopping lane writes its sticky outcome and the zero limit of its
// next step.
extern "C" __global__ void __launch_bounds__(256) hy_step_action(const hy_sa_args a)
{
    const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 N = a.N;
    if (s >= N) return;
    if (a.last_h[s] == 0.0) return;
)HIP";
    src << emit_assignment_section(sec, sec.rows);
    if (sec.has_cond) {
        src << "const bool stop = !(r" << sec.rows.size() << " == 0.0);\n";
        src << R"HIP(const u64 m = __builtin_amdgcn_ballot_w64(stop);
if (stop) {
    if ((unsigned)__builtin_ctzll(m) == (threadIdx.x & 63u)) atomicAdd(a.counter, (unsigned)__builtin_popcountll(m));
    if (a.retired != nullptr) {
        a.retired[s] = HY_SA_CB_STOP;
        a.outcome_w[s] = HY_SA_CB_STOP;
        a.lim[s] = 0.0;
        if (a.gidx != nullptr) a.gidx[s] = a.n_grid;
    }
}
)HIP";
    }
    src << "}\n";
    return src.str();
}

bool callback_is_library_action(const step_callback_batch<double> &cb)
{
    if (cb.extract<step_action>() != nullptr) {
        return true;
    }
    const auto *set = cb.extract<step_callback_batch_set<double>>();
    if (set == nullptr) {
        return false;
    }
    bool any_action = false;
    for (std::size_t i = 0; i < set->size(); ++i) {
        if ((*set)[i].extract<step_action>() != nullptr) {
            any_action = true;
        } else if ((*set)[i].extract<callback::angle_reducer>() == nullptr) {
            return false;
        }
    }
    return any_action;
}

bool prepare_step_actions(tab_core &core, const step_callback_batch<double> &cb)
{
    if (const auto *a = cb.extract<step_action>()) {
        core.prepare_step_action(*a);
    } else if (const auto *set = cb.extract<step_callback_batch_set<double>>()) {
        for (std::size_t i = 0; i < set->size(); ++i) {
            (void)prepare_step_actions(core, (*set)[i]);
        }
    }
    return cb && callback_is_library_action(cb);
}

} // namespace detail

} // namespace heyoka_amd
