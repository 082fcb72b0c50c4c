// Symbolic differentiation and host-side evaluation of expressions.
//
// diff(e, x) mirrors the *semantics* of the reference's diff(expression, expression) for a variable or a parameter
// (reference: include/heyoka/expression.hpp, the gradient() members under src/math/): one rule per built-in func_kind, the
// result memoised on shared nodes through a pointer cache (like rename_variables()), zeros and ones folded by the
// ordinary operators. Functions defined through the registry of node rules (func_kind::custom) have no gradient:
// not_implemented_error naming the function.
//
// eval() is the only host-side evaluator of the expression system: plain recursion with the same memoisation, host libm,
// a Newton solve for kepE. It exists for the tests of diff() and of the variational equations (and for users who want a
// number out of a small expression without a device); the device-side counterpart is cfunc.
#pragma once

#include <cstddef>
#include <string>
#include <unordered_map>
#include <vector>

#include "expression.hpp"

namespace heyoka_amd
{

// d e / d x, x a variable or par[i] (std::invalid_argument otherwise).
expression diff(const expression &e, const expression &x);
// The same with a caller-owned cache (node identity -> derivative): calls which differentiate with respect to the SAME x
// share the derivatives of the nodes they share.
expression diff(ptr_ex_map &cache, const expression &e, const expression &x);

// Value of e with the variables taken from vars (std::invalid_argument for a missing one), par[i] from pars
// (std::invalid_argument if out of range) and heyoka::time = time. not_implemented_error for a custom function.
double eval(const expression &e, const std::unordered_map<std::string, double> &vars, const std::vector<double> &pars = {},
            double time = 0.);

// Number of DISTINCT function nodes (by identity) below the expressions: the size measure of the shared DAG.
std::size_t count_function_nodes(const std::vector<expression> &);

} // namespace heyoka_amd
