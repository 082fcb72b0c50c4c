// Expression sections. See expr_section.hpp.
#include "expr_section.hpp"

#include <algorithm>
#include <set>
#include <stdexcept>

namespace heyoka_amd::detail
{

namespace
{

void check_variables(const expression &ex, std::size_t k, const std::vector<expression> &state_vars, const section_wording &w)
{
    for (const auto &v : get_variables(ex)) {
        if (std::none_of(state_vars.begin(), state_vars.end(), [&](const auto &sv) { return sv.var_name() == v; })) {
            throw std::invalid_argument(w.foreign_variable(k, v));
        }
    }
}

} // namespace

expr_section make_expr_section(const std::vector<expression> &fn, const std::vector<expression> &state_vars, std::uint32_t n_par,
                               const section_wording &w)
{
    for (std::size_t k = 0; k < fn.size(); ++k) {
        check_variables(fn[k], k, state_vars, w);
    }
    expr_section ret;
    const auto dc = function_decompose(fn, state_vars);
    ret.prog = make_program(dc, static_cast<std::uint32_t>(state_vars.size()), static_cast<std::uint32_t>(fn.size()));
    if (ret.prog.n_par > n_par) {
        throw std::invalid_argument(w.par_out_of_range(ret.prog.n_par - 1u, n_par));
    }
    std::set<std::uint32_t> reads;
    const auto visit = [&](const operand &o) {
        if (o.type == operand::kind::uvar && o.idx < ret.prog.n_eq) {
            reads.insert(o.idx);
        }
    };
    for (const auto &n : ret.prog.nodes) {
        std::for_each(n.args.begin(), n.args.end(), visit);
    }
    std::for_each(ret.prog.sv_defs.begin(), ret.prog.sv_defs.end(), visit);
    ret.reads.assign(reads.begin(), reads.end());
    return ret;
}

std::vector<std::uint32_t> assignment_rows(const std::vector<std::pair<expression, expression>> &assignments,
                                           const std::vector<expression> &state_vars, const section_wording &w,
                                           const std::string &kind, const std::string &where)
{
    std::vector<std::uint32_t> rows;
    for (const auto &[lhs, ex] : assignments) {
        const auto it = std::find(state_vars.begin(), state_vars.end(), lhs);
        if (!lhs.is_variable() || it == state_vars.end()) {
            throw std::invalid_argument("The left-hand side '" + lhs.to_string() + "' of an assignment of " + kind
                                        + " is not a state variable of the system" + where);
        }
        const auto row = static_cast<std::uint32_t>(it - state_vars.begin());
        if (std::find(rows.begin(), rows.end(), row) != rows.end()) {
            throw std::invalid_argument("The state variable '" + lhs.to_string() + "' is assigned more than once by " + kind + where);
        }
        check_variables(ex, rows.size(), state_vars, w);
        rows.push_back(row);
    }
    return rows;
}

std::vector<expression> state_variables_of(const std::vector<std::pair<expression, expression>> &sys)
{
    std::vector<expression> ret;
    for (const auto &eq : sys) {
        ret.push_back(eq.first);
    }
    return ret;
}

} // namespace heyoka_amd::detail
