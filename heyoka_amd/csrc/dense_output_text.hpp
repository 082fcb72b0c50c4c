// Dense output from the global buffer of Taylor coefficients: the ONE place where the recurrences which evaluate a system's
// Taylor polynomial from a.tc are spelled, and the kernels made of them - hy_dout (every stepper module), hy_dout_c and
// hy_tc_expand (the companion module of a stepper which stores compact coefficients), hy_dout_rows (the state columns of the
// event log). hy_obs_rows (event_observables.cpp) is assembled from the same pieces: that these kernels agree bit for bit -
// same operations, same order - holds by construction. (The final evaluations INSIDE the steppers read registers or LDS and
// are written by their generators; grid_post.cpp and continuous_output.cpp keep their own raw-string forms.)
//
// The module-level entry points - emit_compact_tc_module(), make_event_log_dout_source() - are declared in hip_emit.hpp.
#pragma once

#include <cstdint>
#include <ostream>
#include <sstream>
#include <string>
#include <vector>

#include "hip_emit.hpp"

namespace heyoka_amd::emit_detail
{

// Is state variable i defined by another state variable (x' = v)? Its Taylor coefficients are then v^[k-1] / k.
bool defined_by_state_variable(const taylor_program &p, std::uint32_t i);

// Compact Taylor coefficients (emit_options::compact_tc): the stepper wrote only the order-0 row of the state variables
// defined by another state variable. Per state variable the row it is derived from and the (last) row derived from it, -1
// for none; empty without compact_tc - then no row is derived.
struct compact_rows {
    std::vector<int> parent, child;
    bool derived(std::uint32_t i) const
    {
        return !parent.empty() && parent[i] >= 0;
    }
};
compact_rows make_compact_rows(const taylor_program &p, const emit_options &opts);

// The coefficient x^[k] of a derived row from the coefficient v^[k-1] of its parent and rk - 1 / k, or k under
// kw::exact_division (rk_value(); as a literal or as an entry of the table hy_rk_c): a product through hy_mul_nc(), which is
// never contracted into an FMA with its consumer - the value must be the ROUNDED product the stepper would have stored,
// whatever comes next (x_1 - x_2, the Horner step) -, or the correctly rounded quotient.
double rk_value(const emit_options &opts, std::uint32_t k);
std::string derived_coeff_text(const emit_options &opts, const std::string &parent_coeff, const std::string &rk);

// What the kernels on compact coefficients need ahead of them: hy_mul_nc(), the table hy_rk_c[order + 1] and - rows != nullptr -
// the tables hy_tc_parent / hy_tc_child of the kernels which loop over the state variables.
void emit_compact_preamble(std::ostream &os, const emit_options &opts, const compact_rows *rows);

// The recurrences. Both read `const double *c` (the coefficients of one state variable of system s, order k at
// c[(u64)k * N]) and the step `h`, and open no scope of their own.
// Full coefficients: defines `res`, the value of the variable at h - Horner, or (high_accuracy) ascending orders with
// compensated summation (reference: taylor_add_d_out_function(), src/taylor_01.cpp:1015-1185).
void emit_plain_recurrence(std::ostream &os, const emit_options &opts);
// Compact coefficients: ONE pass over the coefficients of a stored variable v updates its own sum (want_v: `rv`) and the sums
// of the variables x it defines (x' = v: x^[k] = v^[k-1] / k), with the operations and the operation order of the plain
// recurrence on the full set. Per entry of `kids` a suffix sfx: `x0<sfx>` holds the order-0 coefficient of x, `rx<sfx>` is
// defined as its value at h ("" in the kernels which loop over the variables, "_<i>" where the rows are unrolled).
void emit_compact_recurrence(std::ostream &os, const emit_options &opts, bool want_v, const std::vector<std::string> &kids);

// hy_dout, the dense-output kernel of every stepper module (always on full coefficients).
void emit_dout(std::ostringstream &os, const taylor_program &p, const emit_options &opts);
// The preamble and the kernels hy_dout_c and hy_tc_expand on compact coefficients (opts.compact_tc), without the common
// prelude: the text of emit_compact_tc_module(), which emit_event_jets() puts ahead of hy_ev_jets.
std::string compact_tc_kernels_text(const taylor_program &p, const emit_options &opts);

} // namespace heyoka_amd::emit_detail
