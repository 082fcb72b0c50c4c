// step_action. See step_action.hpp.
#include "step_action.hpp"

#include <algorithm>
#include <ostream>
#include <set>
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

std::vector<expression> state_variables_of(const tab_core::sys_t &sys)
{
    std::vector<expression> ret;
    for (const auto &eq : sys) {
        ret.push_back(eq.first);
    }
    return ret;
}

step_action_section make_step_action_section(const step_action &act, const std::vector<expression> &state_vars,
                                             std::uint32_t n_par)
{
    step_action_section ret;
    std::vector<expression> fn;
    std::set<std::string> names;
    for (const auto &sv : state_vars) {
        names.insert(sv.var_name());
    }
    const auto check_vars = [&](const expression &ex, const std::string &what) {
        for (const auto &v : get_variables(ex)) {
            if (names.count(v) == 0u) {
                throw std::invalid_argument(what + " of a step action uses the variable '" + v
                                            + "', which is not a state variable of the system");
            }
        }
    };
    for (const auto &[lhs, ex] : act.get_assignments()) {
        const auto it = std::find(state_vars.begin(), state_vars.end(), lhs);
        if (!lhs.is_variable() || it == state_vars.end()) {
            throw std::invalid_argument("The left-hand side '" + lhs.to_string()
                                        + "' of an assignment of a step action is not a state variable of the system");
        }
        const auto row = static_cast<std::uint32_t>(it - state_vars.begin());
        if (std::find(ret.rows.begin(), ret.rows.end(), row) != ret.rows.end()) {
            throw std::invalid_argument("The state variable '" + lhs.to_string() + "' is assigned more than once by a step action");
        }
        check_vars(ex, "The right-hand side of the assignment to '" + lhs.to_string() + "'");
        ret.rows.push_back(row);
        fn.push_back(ex);
    }
    if (act.get_stop_when()) {
        check_vars(*act.get_stop_when(), "The stop condition");
        fn.push_back(*act.get_stop_when());
        ret.has_cond = true;
    }
    const auto dc = function_decompose(fn, state_vars);
    ret.prog = make_program(dc, static_cast<std::uint32_t>(state_vars.size()), static_cast<std::uint32_t>(fn.size()));
    if (ret.prog.n_par > n_par) {
        throw std::invalid_argument("A step action uses par[" + std::to_string(ret.prog.n_par - 1u) + "], but the integrator has "
                                    + std::to_string(n_par) + " parameter(s)");
    }
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
    src << emit_assignment_section(p, sec.rows);
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
