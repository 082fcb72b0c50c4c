// Evaluation of the Taylor map of a variational integrator on the device.
//
// For every original state variable i,
//     out_i = sum_alpha s_{i,alpha} * RN(1 / alpha!) * delta^alpha,
// s_{i,alpha} the variational variable (i, alpha) of the state (alpha = 0: the state variable itself), the terms taken in
// the equation order of var_ode_sys (total order, then reverse-lexicographic multi-index) starting from the order-0 term and
// accumulated with fma; the monomials follow the graded schedule delta^alpha = delta^(alpha - e_j) * delta_j, j the highest
// non-zero index of alpha. The host unrolls the schedule into the source: one hiprtc module per (n_orig_sv, n_args, order).
//
// Reference: taylor_adaptive_batch::eval_taylor_map() (src/taylor_adaptive_batch.cpp:2415-2470), which runs a compiled
// function once per batch lane. Two kernels here:
//   hy_tmap        one lane per system, reference layouts in[a * N + sys], out[i * N + sys], the SoA state read in place;
//   hy_tmap_cloud  n_samples displacement vectors per system, sample-fastest layouts
//                  delta[(sys * n_args + a) * n_samples + m] (one cloud shared by all systems: delta[a * n_samples + m]),
//                  out[(sys * n_orig + i) * n_samples + m]; a workgroup serves one system: it stages the system's
//                  pre-scaled coefficients into LDS once and runs its lanes over the samples.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "kernel_args.hpp"

namespace heyoka_amd::detail
{

// The terms of one output, in evaluation order.
struct taylor_map_schedule {
    std::uint32_t n_orig = 0, n_args = 0, order = 0;
    // alpha[t]: dense multi-index of term t (alpha[0] = 0).
    std::vector<std::vector<std::uint32_t>> alpha;
    // parent[t] / last[t]: delta^alpha[t] = delta^alpha[parent[t]] * delta_last[t] (t >= 1; parent 0 is the constant 1).
    std::vector<std::uint32_t> parent, last;
    // RN(1 / alpha[t]!).
    std::vector<double> rfact;
    // first_term[k] / count[k]: the terms of total order k; row_base[k]: the state row of (component 0, first multi-index
    // of order k) - the row of (i, term t of order k) is row_base[k] + i * count[k] + (t - first_term[k]).
    std::vector<std::uint32_t> first_term, count, row_base;

    [[nodiscard]] std::uint32_t n_terms() const
    {
        return static_cast<std::uint32_t>(alpha.size());
    }
    [[nodiscard]] std::uint32_t row(std::uint32_t i, std::uint32_t t) const;
    // Total number of equations of the variational system: n_orig * n_terms.
    [[nodiscard]] std::uint32_t dim() const
    {
        return n_orig * n_terms();
    }
};

taylor_map_schedule make_taylor_map_schedule(std::uint32_t n_orig, std::uint32_t n_args, std::uint32_t order);

// LDS the cloud kernel may use per workgroup for the coefficients of a system: 16 KiB keeps eight 256-lane workgroups
// (the 32 waves a CU can hold) inside the 160 KiB of a CU. HEYOKA_AMD_TMAP_LDS_BYTES overrides it (experiments, and the
// test of the grouped path).
inline constexpr std::size_t taylor_map_default_lds_bytes = 16384;
// What a workgroup can declare statically: the coefficients of ONE output must fit (a group is at least one output).
// make_taylor_map_source() raises not_implemented_error beyond it; an integrator over such a system is constructed without
// the module and its map evaluations raise the same error.
inline constexpr std::size_t taylor_map_max_static_lds_bytes = 65536;
std::size_t taylor_map_lds_bytes();

// HIP source of the module (kernels hy_tmap and hy_tmap_cloud). lds_bytes: the limit above - when the coefficients of a
// system do not fit, the cloud kernel processes the outputs in groups (at least one output per group); *note (may be
// null) receives what was decided, for the stage logger.
std::string make_taylor_map_source(std::uint32_t n_orig, std::uint32_t n_args, std::uint32_t order,
                                   std::size_t lds_bytes = taylor_map_default_lds_bytes, std::string *note = nullptr);

} // namespace heyoka_amd::detail
