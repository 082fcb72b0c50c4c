// HIP source generation. See hip_emit.hpp.
//
// The arithmetic emitted for each node follows the "default mode" formulas of the reference
// (products first, then a pairwise sum; citations next to each rule) so that results agree with
// heyoka's CPU path up to FMA contraction and the <= 1 ulp elementary functions.
#include "hip_emit.hpp"
#include "hip_emit_detail.hpp"
#include "logging.hpp"
#include "taylor_adaptive_batch.hpp"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>

namespace heyoka_amd
{

std::string fp_literal(double x)
{
    if (std::isnan(x)) {
        return "__builtin_nan(\"\")";
    }
    if (std::isinf(x)) {
        return x > 0 ? "__builtin_inf()" : "(-__builtin_inf())";
    }
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%a", x);
    std::string s(buf);
    if (x < 0 || (x == 0 && std::signbit(x))) {
        return "(" + s + ")";
    }
    return s;
}

// NOTE: the modules are compiled with -ffp-contract=fast, under which the backend fuses a product into a following
// difference whatever the pragmas say: the product goes through an empty asm operand, which is opaque to it (like
// hy_mul_nc() of the event-jet module). The quotient is a correctly rounded division (no reciprocal-math flag is ever set).
const char *const angle_reduce_helper_source = R"HIP(
// callback::angle_reducer: x - 2 pi floor(x / 2 pi) with a rounded quotient, product and difference (no contraction);
// non-finite values pass through, so that the non-finite detection of the steppers still sees them.
__device__ __forceinline__ double hy_angle_red(double x)
{
    const double twopi = 0x1.921fb54442d18p+2;
    double q = x / twopi;
    asm("" : "+v"(q));
    double t = twopi * floor(q);
    asm("" : "+v"(t));
    const double r = x - t;
    return (fabs(x) < __builtin_inf()) ? r : x;
}
)HIP";

std::string make_angle_reduce_source()
{
    std::string src = angle_reduce_helper_source;
    src += "\n";
    src += detail::ar_kargs_text();
    src += R"HIP(
extern "C" __global__ void __launch_bounds__(256) hy_angle_reduce(const hy_ar_kargs a)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (t >= a.N * a.n_idx) return;
    const unsigned long long j = t / a.N, s = t - j * a.N;
    double *p = a.state + (unsigned long long)a.idx[j] * a.N + s;
    *p = hy_angle_red(*p);
}
)HIP";
    return src;
}

// Host counterpart of hy_angle_red(): the same three operations, kept apart by volatile temporaries so that no
// compiler setting can contract the product into the difference.
double angle_reduce_host(double x) noexcept
{
    const double twopi = 0x1.921fb54442d18p+2;
    if (!std::isfinite(x)) {
        return x;
    }
    volatile double q = x / twopi;
    volatile double t = twopi * std::floor(q);
    return x - t;
}

emitted_module emit_angle_reduce_variant(const taylor_program &prog, const emit_options &opts, std::string &why_not)
{
    if (opts.angle_reduce.empty() || !std::is_sorted(opts.angle_reduce.begin(), opts.angle_reduce.end())
        || opts.angle_reduce.back() >= prog.n_eq) {
        throw std::invalid_argument("Invalid list of state variables for the fused angle reduction");
    }
    auto m = emit_hip_module(prog, opts);
    if (!m.angle_reduce_fused) {
        why_not = "the generator of this stepper has no fused angle reduction (" + m.notes.substr(0, m.notes.find_first_of(":,;("))
                  + ")";
        return {};
    }
    return m;
}

namespace emit_detail
{

// (The values as taylor_outcome writes them: -2^32 - k.)
std::string outcome_define(const char *name, taylor_outcome oc)
{
    const auto base = -(1ll << 32);
    return std::string("#define ") + name + " (" + std::to_string(base) + "LL - " + std::to_string(base - static_cast<long long>(oc))
           + ")\n";
}

const std::string &prelude()
{
    static const std::string ret = "\ntypedef unsigned long long u64;\ntypedef long long i64;\n\n" + hy_kargs_text() + "\n"
                                   + outcome_define("HY_OC_SUCCESS", taylor_outcome::success)
                                   + outcome_define("HY_OC_STEP_LIMIT", taylor_outcome::step_limit)
                                   + outcome_define("HY_OC_TIME_LIMIT", taylor_outcome::time_limit)
                                   + outcome_define("HY_OC_ERR_NF_STATE", taylor_outcome::err_nf_state) + R"HIP(
// Double-length (hi, lo) arithmetic: Knuth / Dekker error-free transformations
// (reference: include/heyoka/detail/dfloat.hpp:109-164). No multiplications are involved, hence
// FMA contraction cannot alter these sequences; reassociation is never enabled.
struct hy_df {
    double hi, lo;
};

__device__ __forceinline__ hy_df hy_df_add(hy_df a, hy_df b)
{
    const double x_hi = a.hi + b.hi;
    const double z_hi = x_hi - a.hi;
    const double y_hi = (a.hi - (x_hi - z_hi)) + (b.hi - z_hi);
    const double x_lo = a.lo + b.lo;
    const double z_lo = x_lo - a.lo;
    const double y_lo = (a.lo - (x_lo - z_lo)) + (b.lo - z_lo);
    const double w = y_hi + x_lo;
    const double u = x_hi + w;
    const double v = (x_hi - u) + w;
    const double w2 = v + y_lo;
    hy_df r;
    r.hi = u + w2;
    r.lo = (u - r.hi) + w2;
    return r;
}

__device__ __forceinline__ hy_df hy_df_sub(hy_df a, hy_df b)
{
    hy_df nb;
    nb.hi = -b.hi;
    nb.lo = -b.lo;
    return hy_df_add(a, nb);
}

__device__ __forceinline__ bool hy_df_lt(hy_df x, hy_df y)
{
    // NOTE: non-short-circuit operators on purpose (three compares and two mask operations, no control flow).
    return (x.hi < y.hi) | ((x.hi == y.hi) & (x.lo < y.lo));
}

// End-of-step bookkeeping shared by all the steppers (reference: src/taylor_adaptive_batch.cpp:702-727 for the
// outcome of a step, :1402-1460 for the propagate loop): non-finite state check, outcome, step counters, min/max
// step size, remaining time, step limit. Written with selects and ONE (divergent) loop exit instead of a chain of
// early breaks: see the note on HY_LIBM1 about divergent control flow in kernels under register pressure.
// NF: the non-finite flag; COUNT: which thread reports it in the error counter.
#define HY_STEP_TAIL(NF, COUNT)                                                                                        \
    {                                                                                                                  \
        const bool hy_nf = (NF);                                                                                       \
        outcome = hy_nf ? HY_OC_ERR_NF_STATE : ((h == lim) ? HY_OC_TIME_LIMIT : HY_OC_SUCCESS);                       \
        if (hy_nf & (COUNT)) atomicAdd(a.counters, 1u);                                                                \
        bool hy_done = hy_nf | (a.mode != 1);                                                                          \
        n_steps += (!hy_done & (h != 0.0)) ? 1u : 0u;                                                                  \
        const bool hy_upd = !hy_done & (outcome == HY_OC_SUCCESS);                                                     \
        const double hy_ah = fabs(h);                                                                                  \
        min_h = hy_upd ? hy_min(min_h, hy_ah) : min_h;                                                                 \
        max_h = hy_upd ? hy_max(max_h, hy_ah) : max_h;                                                                 \
        hy_done |= (h == rem.hi);                                                                                      \
        {                                                                                                              \
            hy_df hy_tcur;                                                                                             \
            hy_tcur.hi = t_hi;                                                                                         \
            hy_tcur.lo = t_lo;                                                                                         \
            rem = hy_df_sub(tfin, hy_tcur);                                                                            \
        }                                                                                                              \
        ++iter;                                                                                                        \
        const bool hy_sl = !hy_done & (iter == a.max_steps);                                                           \
        outcome = hy_sl ? HY_OC_STEP_LIMIT : outcome;                                                                  \
        hy_done |= hy_sl;                                                                                              \
        if (hy_done) break;                                                                                            \
    }

// x^c for x >= 0, 0 < c < 1: the (1/p)-th roots of the step-size selector (src/taylor_00.cpp:242-252, llvm.pow in
// the reference). exp(log(x) * c) has the same limits (0 -> 0, +inf -> +inf, nan -> nan) and agrees with pow() to
// a few ulps (the error of log(x) is scaled by c < 1), for ~160 instructions less per step than the general-purpose
// device pow().
__device__ __forceinline__ double hy_root(double x, double c)
{
    return exp(log(x) * c);
}

// Logarithm of the step-size selector: written out (45 VALU instructions) instead of the device library's log() (95:
// double-double arithmetic for < 1 ulp) - the selector takes the logarithms of max(1, |x|_inf), |x^[p]|_inf and
// |x^[p-1]|_inf at every step (no quotients: log(num / m) = log(num) - log(m), with the same limits 0 -> +inf,
// inf -> -inf, inf - inf -> nan), which was a sixth of the serial tail of a step of the cluster kernels (there the three
// arguments sit on three lanes of a quad and share ONE evaluation) and 8 % of the two-body stepper. frexp, m in
// [sqrt(1/2), sqrt(2)), z = (m - 1) / (m + 1) by reciprocal + two Newton steps + one residual correction,
// log m = 2 z + z^3 P(z^2) with the Taylor coefficients 2 / (2 n + 1) up to z^21 (|z| <= 0.1716: the first neglected term
// is 2e-17 relative), e ln 2 added in two pieces. Error < 2 ulp (checked against logl on 2e7 arguments); the roots of
// the selector scale it by 1 / p. 0 -> -inf, +inf -> +inf, nan -> nan like log().
__device__ __forceinline__ double hy_sel_log(double x)
{
    double m = __builtin_amdgcn_frexp_mant(x);
    int e = __builtin_amdgcn_frexp_exp(x);
    const bool lo = m < 0x1.6a09e667f3bcdp-1;
    m = m * (lo ? 2.0 : 1.0);
    e -= lo ? 1 : 0;
    const double num = m - 1.0, den = m + 1.0;
    double r = __builtin_amdgcn_rcp(den);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    double z = num * r;
    z = __builtin_fma(__builtin_fma(-den, z, num), r, z);
    const double w = z * z;
    double p = 0x1.8618618618618p-4;
    p = __builtin_fma(p, w, 0x1.af286bca1af28p-4);
    p = __builtin_fma(p, w, 0x1.e1e1e1e1e1e1ep-4);
    p = __builtin_fma(p, w, 0x1.1111111111111p-3);
    p = __builtin_fma(p, w, 0x1.3b13b13b13b14p-3);
    p = __builtin_fma(p, w, 0x1.745d1745d1746p-3);
    p = __builtin_fma(p, w, 0x1.c71c71c71c71cp-3);
    p = __builtin_fma(p, w, 0x1.2492492492492p-2);
    p = __builtin_fma(p, w, 0x1.999999999999ap-2);
    p = __builtin_fma(p, w, 0x1.5555555555555p-1);
    const double ed = (double)e;
    double res = __builtin_fma(ed, 0x1.abc9e3b39803fp-56, (z * w) * p);
    res = __builtin_fma(2.0, z, res);
    res = __builtin_fma(ed, 0x1.62e42fefa39efp-1, res);
    res = (x == 0.0) ? -__builtin_inf() : res;
    res = (x == __builtin_inf()) ? x : res;
    return res;
}

// Out-of-line calls for the math-library functions with data-dependent control flow in their device implementations
// (the Payne-Hanek branch of sin/cos/tan, the piecewise ranges of erf, ...). Inlined into a straight-line kernel with
// several hundred live registers, those divergent if/else regions are where the register allocator splits long live
// ranges, and with this toolchain (ROCm 7.2) such a split can land in the exec-masked flow block between the two sides
// of the branch: the copy is then executed only by the lanes which took the first side and the other lanes read
// stale registers later on (observed as wild jet addresses in a 3500-statement kernel with tan()). As functions of
// their own, the branches live in a small frame without register pressure and the kernel sees an ordinary call at
// its current exec mask. One call per function instance and step (order 0 only): the cost is not measurable.
#define HY_LIBM1(f)                                                                                                    \
    static __device__ __attribute__((noinline)) double hy_##f(double x)                                                \
    {                                                                                                                  \
        return f(x);                                                                                                   \
    }
HY_LIBM1(sin)
HY_LIBM1(cos)
HY_LIBM1(tan)
HY_LIBM1(tanh)
HY_LIBM1(sinh)
HY_LIBM1(cosh)
HY_LIBM1(erf)
HY_LIBM1(asin)
HY_LIBM1(acos)
HY_LIBM1(atan)
HY_LIBM1(asinh)
HY_LIBM1(acosh)
HY_LIBM1(atanh)
#undef HY_LIBM1
static __device__ __attribute__((noinline)) double hy_pow(double x, double y)
{
    return pow(x, y);
}

static __device__ __attribute__((noinline)) double hy_atan2(double y, double x)
{
    return atan2(y, x);
}

// Inverse of Kepler's equation for the eccentric anomaly: E - e sin E = M (reference: llvm_add_inv_kep_E(),
// src/detail/llvm_helpers_celmec.cpp:181-466). Invalid eccentricities (nan, < 0, >= 1) give nan; M is reduced to
// [0, 2 pi) in double-length arithmetic (llvm_trig_arg_reduce(), :140-177, on top of the Dekker / NTL procedures of
// src/detail/llvm_helpers_dl.cpp:130-281); third-order initial guess in e; Newton-Raphson iterations safeguarded by
// bisection on a bracketing interval, stopped when |f(E)| or the bracket are below 4 eps, nan after 20 iterations
// without convergence. One lane per system: every lane stops at its own convergence (the scalar flavour of the
// reference; its batch flavour keeps iterating all the lanes until the slowest has converged, which moves the
// others by rounding errors at most).
static __device__ __attribute__((noinline)) double hy_kepE(double ecc_in, double M_in)
{
#pragma clang fp contract(off)
    const double qnan = __builtin_nan("");
    const bool ecc_invalid = !(ecc_in >= 0.0) | (ecc_in >= 1.0);
    const double ecc = ecc_invalid ? qnan : ecc_in;

    // ---- M mod 2 pi: x - y * floor(x / y) in double-length arithmetic.
    const double y_hi = 0x1.921fb54442d18p+2, y_lo = 0x1.1a62633145c07p-52;
    const double twopi_prev = 0x1.921fb54442d17p+2; // the double preceding 2 pi
    double M;
    {
        // x / y (div2()).
        const double c = M_in / y_hi;
        const double u = c * y_hi, uu = fma(c, y_hi, -u);
        double cc = M_in - u;
        cc = cc - uu;
        cc = cc + 0.0;
        cc = cc - c * y_lo;
        cc = cc / y_hi;
        const double q_hi = c + cc, q_lo = (c - q_hi) + cc;
        // floor().
        const double fhi = floor(q_hi);
        const double flo = (fhi == q_hi) ? floor(q_lo) : 0.0;
        const double fl_hi = fhi + flo, fl_lo = (fhi - fl_hi) + flo;
        // y * floor (mul2()).
        const double pc = y_hi * fl_hi;
        double pcc = fma(y_hi, fl_hi, -pc);
        pcc = (y_hi * fl_lo + y_lo * fl_hi) + pcc;
        const double p_hi = pc + pcc, p_lo = (pc - p_hi) + pcc;
        // x - y * floor.
        hy_df xx, yy;
        xx.hi = M_in;
        xx.lo = 0.0;
        yy.hi = -p_hi;
        yy.lo = -p_lo;
        M = hy_df_add(xx, yy).hi;
        M = (M < 0.0) ? 0.0 : M;
        M = (twopi_prev < M) ? twopi_prev : M;
    }

    // ---- Initial guess: E = M + e sin M + e^2 sin M cos M + e^3 sin M (3/2 cos^2 M - 1/2).
    double sE = sin(M), cE = cos(M);
    double E;
    {
        const double e_sin = ecc * sE, e_cos = ecc * cE, e2 = ecc * ecc, cos2 = cE * cE;
        const double ig1 = (M + e_sin) + e_sin * e_cos;
        const double ig2 = (e2 * e_sin) * (1.5 * cos2 - 0.5);
        E = ig1 + ig2;
    }
    double lb = 0.0, ub = twopi_prev;
    E = (E < lb) ? lb : E;
    E = (ub < E) ? ub : E;
    sE = sin(E);
    cE = cos(E);
    double fE = (E - M) - ecc * sE;

    const double tol = 4.0 * 0x1p-52;
    bool not_converged = false;
    unsigned it = 0;
    for (;;) {
        // Bracket update from the sign of f(E) (0 for nan: the bracket collapses and the loop ends).
        const int sgn = (0.0 < fE) - (fE < 0.0);
        const double n_ub = (sgn >= 0) ? E : ub, n_lb = (sgn <= 0) ? E : lb;
        ub = n_ub;
        lb = n_lb;
        not_converged = (fabs(fE) > tol) & ((ub - lb) > tol);
        if (!(it < 20u) | !not_converged) {
            break;
        }
        // Newton-Raphson step, replaced by a bisection when it leaves the bracket.
        double nE = E - fE / (1.0 - ecc * cE);
        nE = (nE > ub) ? 0.5 * (E + ub) : nE;
        nE = (nE < lb) ? 0.5 * (E + lb) : nE;
        E = nE;
        sE = sin(E);
        cE = cos(E);
        fE = (E - M) - ecc * sE;
        ++it;
    }
    return (it == 20u && not_converged) ? qnan : E;
}

// max(a, b) = (a < b) ? b : a and min(a, b) = (b < a) ? b : a
// (reference: src/detail/llvm_helpers_cmp.cpp:315-329; NaN handling is part of the semantics).
__device__ __forceinline__ double hy_max(double a, double b)
{
    return (a < b) ? b : a;
}
__device__ __forceinline__ double hy_min(double a, double b)
{
    return (b < a) ? b : a;
}

__device__ __forceinline__ bool hy_finite(double x)
{
    return __builtin_isfinite(x);
}
)HIP";
    return ret;
}

// The bookkeeping around a step, once for the steppers with one system-loop and one step-loop per kernel (unrolled, first
// wave-cluster generator, block, HBM-tape table, staged table): the step / propagate_until contract of the reference for
// hy_kargs::mode 0 (one step, limit a.lim), 1 (propagate to tfin, a.lim the optional max_delta_t), 2 (raw stepper) and
// 4 (stepper with events: the caller leaves the loop before HY_STEP_ADVANCE and stores last_h alone). The end of a step is
// HY_STEP_TAIL in prelude(); this block stays out of prelude() because the auxiliary kernels include that and not this.
// Every stepper writes it right behind prelude(). The fragments share their local names (a, t_hi, t_lo, h, lim, rem, tfin,
// ...) with HY_STEP_TAIL and with each other, so they are macros, not functions. The pipelined / pair generator
// (hip_emit_cluster2*.cpp) has a loop of another shape and does not use them.
const std::string &step_loop_source()
{
    static const std::string ret = R"HIP(
// Is the remaining time non-negative (reference: src/taylor_adaptive_batch.cpp:1272)? Two spellings which compile to
// different code: the staged table stepper uses HY_DIR_SELECT, the other four HY_DIR_BRANCHY. Which stepper has which is
// what its code object was built from before the fragments were shared, not a preference: changing one changes a kernel.
#define HY_DIR_BRANCHY(R) (((R).hi > 0.0) || ((R).hi == 0.0 && (R).lo >= 0.0))
#define HY_DIR_SELECT(R) (((R).hi > 0.0) | (((R).hi == 0.0) & ((R).lo >= 0.0)))

// Limits of system S (reference: src/taylor_adaptive_batch.cpp:1264-1273): mode 1 - final time, remaining time, direction
// and the optional max_delta_t; any other mode - the signed limit of the single step.
#define HY_STEP_LIMITS(S, DIR)                                                                                         \
    hy_df tfin, rem;                                                                                                   \
    tfin.hi = 0.0; tfin.lo = 0.0; rem.hi = 0.0; rem.lo = 0.0;                                                          \
    bool t_dir = true;                                                                                                 \
    double mdt = __builtin_inf();                                                                                      \
    double step_lim = 0.0;                                                                                             \
    if (a.mode == 1) {                                                                                                 \
        tfin.hi = (a.tfin_hi != nullptr) ? a.tfin_hi[S] : a.tfin_s_hi;                                                 \
        tfin.lo = (a.tfin_hi != nullptr) ? a.tfin_lo[S] : a.tfin_s_lo;                                                 \
        hy_df tcur; tcur.hi = t_hi; tcur.lo = t_lo;                                                                    \
        rem = hy_df_sub(tfin, tcur);                                                                                   \
        t_dir = DIR(rem);                                                                                              \
        if (a.lim != nullptr) mdt = a.lim[S];                                                                          \
    } else {                                                                                                           \
        step_lim = a.lim[S];                                                                                           \
    }

// What HY_STEP_TAIL counts.
#define HY_STEP_COUNTERS                                                                                               \
    u64 n_steps = 0, iter = 0;                                                                                         \
    double min_h = __builtin_inf(), max_h = 0.0, last_h = 0.0;                                                         \
    i64 outcome = HY_OC_SUCCESS;

// Time limit for this step (reference: src/taylor_adaptive_batch.cpp:1378-1387).
// NOTE: selects, not an if/else on the (per-lane) direction: see the note on HY_LIBM1.
#define HY_STEP_LIM                                                                                                    \
    double lim;                                                                                                        \
    if (a.mode == 1) {                                                                                                 \
        hy_df m; m.lo = 0.0;                                                                                           \
        m.hi = t_dir ? mdt : -mdt;                                                                                     \
        const bool lt_fwd = hy_df_lt(rem, m), lt_bwd = hy_df_lt(m, rem);                                               \
        const bool rem_first = (t_dir & lt_fwd) | (!t_dir & lt_bwd);                                                   \
        lim = rem_first ? rem.hi : m.hi;                                                                               \
    } else {                                                                                                           \
        lim = step_lim;                                                                                                \
    }

// Step size from the infinity norms m0, mo, mom1 of the orders 0, p, p - 1 and the limit (taylor_determine_h(),
// src/taylor_00.cpp:102-273). INV_P = 1 / p, INV_PM1 = 1 / (p - 1), RHOFAC = emit_detail::rhofac(p).
#define HY_STEP_SIZE(INV_P, INV_PM1, RHOFAC)                                                                           \
    const double num_rho = (m0 <= 1.0) ? 1.0 : m0;                                                                     \
    const double rho_o = hy_root(num_rho / mo, INV_P);                                                                 \
    const double rho_om1 = hy_root(num_rho / mom1, INV_PM1);                                                           \
    const double rho_m = hy_min(rho_o, rho_om1);                                                                       \
    double h = rho_m * RHOFAC;                                                                                         \
    h = hy_min(h, fabs(lim));                                                                                          \
    h = (lim < 0.0) ? -h : h;

// The time after the step, in double-length arithmetic (reference: src/taylor_adaptive_batch.cpp:702-727).
#define HY_STEP_ADVANCE                                                                                                \
    {                                                                                                                  \
        hy_df tcur; tcur.hi = t_hi; tcur.lo = t_lo;                                                                    \
        hy_df hh; hh.hi = h; hh.lo = 0.0;                                                                              \
        const hy_df nt = hy_df_add(tcur, hh);                                                                          \
        t_hi = nt.hi; t_lo = nt.lo;                                                                                    \
    }                                                                                                                  \
    last_h = h;

// The results of system S, the state apart; which lanes store them is the caller's business. Raw stepper ABI (mode 2):
// the time is left alone and the step taken is returned through the (in/out) limits array.
#define HY_STEP_RESULT(S)                                                                                              \
    if (a.mode != 2) {                                                                                                 \
        a.time_hi[S] = t_hi;                                                                                           \
        a.time_lo[S] = t_lo;                                                                                           \
    } else {                                                                                                           \
        const_cast<double *>(a.lim)[S] = last_h;                                                                       \
    }                                                                                                                  \
    a.last_h[S] = last_h;                                                                                              \
    a.outcome[S] = outcome;                                                                                            \
    if (a.mode == 1) {                                                                                                 \
        a.min_h[S] = min_h;                                                                                            \
        a.max_h[S] = max_h;                                                                                            \
        a.n_steps[S] = n_steps;                                                                                        \
    }
)HIP";
    return ret;
}

// Scaling + safety factor of the step-size selector, folded on the host in double precision
// (reference: taylor_determine_h_rhofac(), src/taylor_00.cpp:84-94).
double rhofac(std::uint32_t order)
{
    const double m7_10 = -7. / 10.;
    const double e2 = std::exp(1.) * std::exp(1.);
    return std::exp(m7_10 / static_cast<double>(order - 1u)) / e2;
}

// One system per lane, fully unrolled SSA code (the GPU analogue of the reference's default mode,
// taylor_compute_jet() src/taylor_02.cpp:1339-1418).
// One stepper kernel. reg_jets = false: the jets of the state variables go through the tc buffer (always
// needed, also serves kw::write_tc). reg_jets = true: they stay in SSA values (registers); state variables
// defined by other state variables (x' = v) are re-derived in the final evaluation instead of being stored.
// stream_tc (with reg_jets): the Taylor coefficients are additionally streamed to a.tc as they are produced (stores
// only, nothing is read back): the write_tc / continuous-output / propagate_grid variant of a register-resident stepper.
// The u variables whose coefficient HISTORY is read (operands of convolutions and of recurrences, functions with a
// recurrence on themselves): what a lane of the straight-line stepper keeps through the orders.
// (folded: with ssa_emitter::fold_scaled / fold_zeros a history which is a scaled copy of another one - prod(number, u) -, or
// its coefficients beyond order 0 - u + number, u - number -, is not kept: the mark moves to u.)
std::vector<char> history_operands(const taylor_program &p, bool folded = false)
{
    std::vector<char> hist(p.n_u, 0);
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        const auto &nd = p.nodes[i];
        const auto &a = nd.args;
        const auto mark = [&](const operand &o) {
            if (o.type == operand::kind::uvar) {
                hist[o.idx] = 1;
            }
        };
        switch (nd.kind) {
            case func_kind::prod:
                if (a.size() == 2u && a[0].type == operand::kind::uvar && a[1].type == operand::kind::uvar) {
                    mark(a[0]);
                    mark(a[1]);
                }
                break;
            case func_kind::sum_sq:
                for (const auto &o : a) {
                    mark(o);
                }
                break;
            case func_kind::pow:
            case func_kind::exp:
            case func_kind::log:
            case func_kind::sin:
            case func_kind::cos:
                if (a[0].type == operand::kind::uvar) {
                    mark(a[0]);
                    // (The square is a convolution of its argument with itself: no recurrence on its own coefficients.)
                    const bool square = nd.kind == func_kind::pow && a.size() == 2u && a[1].type == operand::kind::num && a[1].value == 2.;
                    if (!(folded && square)) {
                        hist[p.n_eq + i] = 1;
                    }
                }
                break;
            case func_kind::div:
                if (a[1].type == operand::kind::uvar) {
                    mark(a[1]);
                    hist[p.n_eq + i] = 1;
                }
                break;
            default:
                break;
        }
    }
    for (std::uint32_t i = static_cast<std::uint32_t>(p.nodes.size()); folded && i-- > 0u;) {
        const auto &nd = p.nodes[i];
        const auto &a = nd.args;
        if (hist[p.n_eq + i] == 0) {
            continue;
        }
        std::uint32_t n_var = 0, parent = 0;
        for (const auto &o : a) {
            if (o.type == operand::kind::uvar) {
                ++n_var;
                parent = o.idx;
            }
        }
        const bool copy = n_var == 1u
                          && ((nd.kind == func_kind::prod && a.size() == 2u) || nd.kind == func_kind::sum
                              || (nd.kind == func_kind::sub && a[0].type == operand::kind::uvar));
        if (copy) {
            hist[p.n_eq + i] = 0;
            hist[parent] = 1;
        }
    }
    return hist;
}

// (waves: amdgpu_waves_per_eu of the kernel, 0 = the compiler's choice; n_derived: the number of state variables whose
// coefficient histories are not kept because they are re-derived at the end of the step - see "The other way round" below.)
std::string emit_unrolled_kernel(const taylor_program &p, const emit_options &opts, const std::string &kname,
                                 bool reg_jets, std::uint64_t &n_stmt, bool stream_tc = false, int waves = 0,
                                 std::uint32_t *n_derived = nullptr)
{
    const auto n_eq = p.n_eq;
    const auto order = opts.order;
    const auto bs = opts.block_size;

    ssa_emitter e(p, order);
    auto &os = e.os;
    // Fused callback::angle_reducer (emit_options::angle_reduce): the updated value of a flagged state variable goes
    // through hy_angle_red() before it is checked, stored or reused.
    const auto reduced = [&](std::uint32_t i, const std::string &v) {
        return std::binary_search(opts.angle_reduce.begin(), opts.angle_reduce.end(), i) ? ("hy_angle_red(" + v + ")") : v;
    };
    e.enable_pow_rcp(!opts.exact_division);
    e.running_sums = opts.sum_order != 1;
    // Divisions by the (constant) order: one multiplication by RN(1 / k), within 1 ulp of the quotient (like the pair
    // kernels), unless kw::exact_division asks for the correctly rounded 3-operation sequence - 120 of them per step of
    // the two-body problem.
    e.recip_div = !opts.exact_division;
    e.fold_zeros = opts.dev.unrolled_trim;
    e.fold_scaled = opts.dev.unrolled_trim && !opts.exact_division && opts.sum_order == 0;
    e.merge_sum_sq = opts.sum_order == 0 && !opts.exact_division && opts.dev.unrolled_merge_ssq;

    os << "extern \"C\" __global__ void __launch_bounds__(" << bs << ") ";
    if (waves > 0) {
        os << "__attribute__((amdgpu_waves_per_eu(" << waves << ", " << waves << "))) ";
    }
    os << kname << "(const hy_kargs a)\n{\n";
    os << "const u64 s = (u64)blockIdx.x * " << bs << "u + threadIdx.x;\n";
    os << "if (s >= a.N) return;\n";
    os << "const u64 N = a.N;\n";
    os << "double t_hi = a.time_hi[s], t_lo = a.time_lo[s];\n";
    for (std::uint32_t i = 0; i < p.n_par; ++i) {
        os << "const double par_" << i << " = a.pars[(u64)" << i << "u * N + s];\n";
    }
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        os << "double x" << i << " = a.state[(u64)" << i << "u * N + s];\n";
        if (reg_jets) {
            os << "double x" << i << "n = 0.0;\n";
        }
    }
    if (stream_tc) {
        os << "double *jet = a.tc + s;\n";
    } else if (!reg_jets) {
        os << "double *jet = a.tc + s;\n";
    }
    os << "HY_STEP_LIMITS(s, HY_DIR_BRANCHY)\nHY_STEP_COUNTERS\nfor (;;) {\nHY_STEP_LIM\n";
    if (stream_tc || !reg_jets) {
        // NOTE: the (order + 1) * n_eq store addresses are invariants of the step loop: left alone, the compiler hoists
        // all of them into registers (2 per address). Laundering the base pointer once per step makes them per-step values.
        // (Round 6: also in the kernel which keeps the jets of the state variables in memory - cr3bp: 526 -> 0 spilled
        // registers together with the folded histories, see ssa_emitter::fold_scaled.)
        os << "asm volatile(\"\" : \"+v\"(jet));\n";
        // (The same for the scalar halves of the addresses, index * N: hoisted, they are 2 SGPRs each - 651 spilled SGPRs in the
        // stepper of two massive bodies.)
        os << "u64 hy_Ns = N;\n#if defined(HY_HOST_EMU)\nasm volatile(\"\" : \"+r\"(hy_Ns));\n#else\nasm volatile(\"\" : "
              "\"+s\"(hy_Ns));\n#endif\n";
    }

    // ---- Jet of normalised derivatives. ----
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        e.val(i, 0) = "x" + std::to_string(i);
    }
    const auto store_sv = [&](std::uint32_t i, std::uint32_t k) {
        if (reg_jets && !stream_tc) {
            return;
        }
        os << "jet[(u64)" << (static_cast<std::uint64_t>(i) * (order + 1u) + k) << "u * hy_Ns] = " << e.val(i, k)
           << ";\n";
    };
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        store_sv(i, 0);
    }
    for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
        e.node(i, 0);
    }
    // x' = v, v' = u with a v which no elementary function reads (register-resident jets, not under kw::exact_division):
    // x^[k] = u^[k-2] RN(1 / (k (k - 1))) - one multiplication instead of the two through v^[k-1], whose only other use is
    // the final evaluation (where it is re-derived from x, see below; the compiler drops the unused ones).
    std::vector<std::int64_t> second_order(n_eq, -1);
    if (reg_jets && opts.dev.unrolled_derive && !opts.exact_division) {
        std::vector<char> read_by_node(n_eq, 0);
        for (const auto &nd : p.nodes) {
            for (const auto &o : nd.args) {
                if (o.type == operand::kind::uvar && o.idx < n_eq) {
                    read_by_node[o.idx] = 1;
                }
            }
        }
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            const auto &d = p.sv_defs[i];
            if (d.type == operand::kind::uvar && d.idx < n_eq && read_by_node[d.idx] == 0) {
                const auto &dd = p.sv_defs[d.idx];
                if (dd.type == operand::kind::uvar && dd.idx >= n_eq) {
                    second_order[i] = dd.idx;
                }
            }
        }
    }
    const auto emit_sv = [&](std::uint32_t i, std::uint32_t k) {
        if (k >= 2u && second_order[i] >= 0) {
            const auto &src = e.val(static_cast<std::uint32_t>(second_order[i]), k - 2u);
            e.val(i, k) = ssa_emitter::is_zero_lit(src)
                              ? std::string("0.0")
                              : e.def(ssa_emitter::mul(src, fp_literal(1. / (static_cast<double>(k) * static_cast<double>(k - 1u)))));
        } else {
            e.sv(i, k);
        }
        store_sv(i, k);
    };
    for (std::uint32_t k = 1; k < order; ++k) {
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            emit_sv(i, k);
        }
        for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
            e.node(i, k);
        }
    }
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        emit_sv(i, order);
    }

    // Integrators with events: every step is a step with events (mode 4), which needs the order-p coefficients of the u
    // variables (src/taylor_02.cpp:1016-1190) - and the event equations take part in the norms of the step-size
    // selector (taylor_determine_h() iterates up to n_eq + n_sv_funcs, src/taylor_00.cpp:209-219), so that the step
    // stays inside the convergence radius of their Taylor series as well.
    const bool ev_norms = !p.ev_u.empty() && !reg_jets;
    if (ev_norms) {
        for (std::uint32_t i = 0; i < p.nodes.size(); ++i) {
            e.node(i, order);
        }
    }

    // ---- Step size (reference: taylor_determine_h(), src/taylor_00.cpp:102-273). ----
    const auto max_abs = [&](std::uint32_t k) {
        std::vector<std::string> v;
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            v.push_back(e.def("fabs(" + e.val(i, k) + ")"));
        }
        if (ev_norms) {
            for (const auto u : p.ev_u) {
                v.push_back(e.def("fabs(" + e.val(u, k) + ")"));
            }
        }
        while (v.size() != 1u) {
            std::vector<std::string> nv;
            for (std::size_t i = 0; i < v.size(); i += 2u) {
                if (i + 1u == v.size()) {
                    nv.push_back(v[i]);
                } else {
                    nv.push_back(e.def("hy_max(" + v[i] + ", " + v[i + 1u] + ")"));
                }
            }
            v.swap(nv);
        }
        return v[0];
    };
    const auto m0 = max_abs(0), mo = max_abs(order), mom1 = max_abs(order - 1u);
    os << "const double num_rho = (" << m0 << " <= 1.0) ? 1.0 : " << m0 << ";\n";
    // rho = exp(log(num / m) / order) (the (1/p)-th roots of src/taylor_00.cpp:242-252): the minimum of the two estimates
    // is taken on the exponents (exp is monotone and keeps nans), the quotients become differences of logarithms.
    os << "const double lg_num = hy_sel_log(num_rho);\n";
    os << "const double lr_o = (lg_num - hy_sel_log(" << mo << ")) * " << fp_literal(1. / static_cast<double>(order)) << ";\n";
    os << "const double lr_om1 = (lg_num - hy_sel_log(" << mom1 << ")) * " << fp_literal(1. / static_cast<double>(order - 1u))
       << ";\n";
    os << "const double rho_m = exp(hy_min(lr_o, lr_om1));\n";
    os << "double h = rho_m * " << fp_literal(rhofac(order)) << ";\n";
    os << "h = hy_min(h, fabs(lim));\n";
    os << "h = (lim < 0.0) ? -h : h;\n";

    if (!p.ev_u.empty() && !reg_jets) {
        // ---- Stepper with events (mode 4; taylor_add_adaptive_step_with_events(), src/taylor_00.cpp:592-710): the
        // order-p coefficients of the u variables (src/taylor_02.cpp:1016-1190), the jets of the event equations,
        // max |x_i| and the step size; the state is updated later by the dense-output kernel.
        os << "if (a.mode == 4) {\n";
        for (std::size_t ev = 0; ev < p.ev_u.size(); ++ev) {
            for (std::uint32_t k = 0; k <= order; ++k) {
                os << "a.ev_tc[(u64)" << (ev * (order + 1u) + k) << "u * N + s] = " << e.val(p.ev_u[ev], k) << ";\n";
            }
        }
        os << "a.max_abs_state[s] = " << m0 << ";\nlast_h = h;\nbreak;\n}\n";
    }

    if (reg_jets) {
        // ---- State update straight from the SSA coefficients. ----
        // Coefficient k of state variable i: re-derived from the defining state variable when x' = v.
        // The other way round for a variable v which only DEFINES another one (x' = v, no elementary function reads v) when
        // the coefficients of x are live anyway (they are the coefficients of a u variable with a history: x^[k] = d^[k]
        // where the partner of the difference d has vanishing derivatives - a test particle): v^[k] = (k + 1) x^[k+1], one
        // multiplication at the end of the step instead of a coefficient history through the orders (two-body problem:
        // 3 of 8 histories). Within 1.5 ulp of the coefficient (x^[k+1] = RN(v^[k] RN(1 / (k + 1)))): not under
        // kw::exact_division.
        std::set<std::string> hist_names;
        std::vector<std::int64_t> defines(n_eq, -1);
        if (opts.dev.unrolled_derive && !opts.exact_division) {
            std::vector<char> read_by_node(n_eq, 0);
            for (const auto &nd : p.nodes) {
                for (const auto &o : nd.args) {
                    if (o.type == operand::kind::uvar && o.idx < n_eq) {
                        read_by_node[o.idx] = 1;
                    }
                }
            }
            // (Names of the coefficients which are kept anyway: the histories.)
            const auto hist = history_operands(p);
            for (std::uint32_t u = 0; u < p.n_u; ++u) {
                for (std::uint32_t k = 0; hist[u] != 0 && k <= order; ++k) {
                    hist_names.insert(e.val(u, k));
                }
            }
            for (std::uint32_t j = 0; j < n_eq; ++j) {
                const auto &d = p.sv_defs[j];
                if (d.type == operand::kind::uvar && d.idx < n_eq && read_by_node[d.idx] == 0) {
                    defines[d.idx] = (defines[d.idx] == -1) ? static_cast<std::int64_t>(j) : -2;
                }
            }
        }
        std::vector<std::uint32_t> derived_count(n_eq, 0);
        // (v is re-derived from x when x is the one variable it defines and the coefficients of x are those of a history -
        // checked on order 2, the first one which is not a plain copy of another state variable.)
        const auto derive_v = [&](std::uint32_t v) {
            return order >= 3u && defines[v] >= 0 && hist_names.count(e.val(static_cast<std::uint32_t>(defines[v]), 2u)) != 0u;
        };
        std::function<std::string(std::uint32_t, std::uint32_t)> coef = [&](std::uint32_t i, std::uint32_t k) {
            const auto &d = p.sv_defs[i];
            if (k > 0u && d.type == operand::kind::uvar && d.idx < n_eq) {
                if (derive_v(d.idx)) {
                    // (Never back from the re-derived v.)
                    return e.val(i, k);
                }
                return e.div_const(coef(d.idx, k - 1u), k);
            }
            if (k > 0u && k < order && derive_v(i)) {
                const auto &xk = e.val(static_cast<std::uint32_t>(defines[i]), k + 1u);
                if (!ssa_emitter::is_zero_lit(xk)) {
                    ++derived_count[i];
                    return e.def(ssa_emitter::mul(fp_literal(static_cast<double>(k + 1u)), xk));
                }
            }
            return e.val(i, k);
        };
        // A pair x' = v with a re-derived v, plain Horner evaluation: sum_k (k + 1) x^[k+1] h^k is the DERIVATIVE of the series
        // of x - both come out of one pass (res' = res' h + res, res = res h + x^[k]: two FMAs per coefficient, like the two
        // chains) without the multiplications by k + 1; the term v^[p] h^p, which the series of x knows nothing of, is added at
        // the end (h^p by squaring, once per step).
        std::vector<char> paired(n_eq, 0);
        std::string h_to_p;
        for (std::uint32_t v = 0; v < n_eq && !opts.high_accuracy && opts.dev.unrolled_derive; ++v) {
            if (!derive_v(v)) {
                continue;
            }
            const auto x = static_cast<std::uint32_t>(defines[v]);
            bool ok = true;
            for (std::uint32_t k = 2; k <= order; ++k) {
                ok = ok && !ssa_emitter::is_zero_lit(e.val(x, k)) && !e.val(x, k).empty();
            }
            if (!ok) {
                continue;
            }
            if (h_to_p.empty()) {
                h_to_p = e.pow_ebs("h", order);
            }
            // (x^[1] = v^[0] / 1 = the current v; x^[0] = the current x.)
            os << "{\ndouble res = " << e.val(x, order) << ", der = " << e.val(x, order) << ";\n";
            os << "res = " << e.val(x, order - 1u) << " + res * h;\n";
            for (std::uint32_t k = order - 1u; k-- > 0u;) {
                os << "der = res + der * h;\nres = " << coef(x, k) << " + res * h;\n";
            }
            os << "x" << x << "n = res;\nx" << v << "n = " << e.val(v, order) << " * " << h_to_p << " + der;\n}\n";
            paired[x] = paired[v] = 1;
            derived_count[v] = order - 1u;
        }
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            if (paired[i] != 0) {
                continue;
            }
            if (opts.high_accuracy) {
                os << "{\ndouble res = " << coef(i, 0) << ", comp = 0.0, cur_h = h;\n";
                for (std::uint32_t k = 1; k <= order; ++k) {
                    const auto c = coef(i, k);
                    os << "{\nconst double tmp = " << c << " * cur_h;\nconst double y = tmp - comp;\n";
                    os << "const double t = res + y;\ncomp = (t - res) - y;\nres = t;\ncur_h = cur_h * h;\n}\n";
                }
                os << "x" << i << "n = res;\n}\n";
            } else {
                // NOTE: coefficients are named before the block so that the chain is a pure Horner recursion.
                std::vector<std::string> cs;
                for (std::uint32_t k = 0; k <= order; ++k) {
                    cs.push_back(coef(i, k));
                }
                // Leading coefficients which are the literal +0 (derivatives which vanish identically): the steps
                // res = 0 + res * h over them yield +0 for a finite h and a NaN otherwise from the first one on - ONE of them
                // is all of them (the compiler cannot drop any: no fast-math flags).
                std::uint32_t top = order;
                if (opts.dev.unrolled_trim) {
                    while (top >= 1u && ssa_emitter::is_zero_lit(cs[top]) && ssa_emitter::is_zero_lit(cs[top - 1u])) {
                        --top;
                    }
                }
                os << "{\ndouble res = " << cs[top] << ";\n";
                for (std::uint32_t k = order - top + 1u; k <= order; ++k) {
                    os << "res = " << cs[order - k] << " + res * h;\n";
                }
                os << "x" << i << "n = res;\n}\n";
            }
        }
        for (std::uint32_t i = 0; i < n_eq; ++i) {
            os << "x" << i << " = " << reduced(i, "x" + std::to_string(i) + "n") << ";\n";
        }
        if (n_derived != nullptr) {
            *n_derived = static_cast<std::uint32_t>(
                std::count_if(derived_count.begin(), derived_count.end(), [&](std::uint32_t c) { return c + 1u == order; }));
        }
    } else {
        // ---- State update: reload the coefficients from the jet buffer. ----
        // NOTE: the memory clobber prevents the compiler from forwarding the stored coefficients (which
        // would keep (order + 1) * n_eq values live in registers across the whole step).
        os << "asm volatile(\"\" ::: \"memory\");\n";
        if (opts.high_accuracy) {
            // Compensated summation (reference: taylor_run_ceval(), src/taylor_00.cpp:355-460).
            for (std::uint32_t i = 0; i < n_eq; ++i) {
                os << "{\nconst double *c = jet + (u64)" << (static_cast<std::uint64_t>(i) * (order + 1u))
                   << "u * hy_Ns;\n";
                os << "double res = c[0], comp = 0.0, cur_h = h;\n";
                os << "#pragma unroll\nfor (unsigned k = 1; k <= " << order << "u; ++k) {\n";
                os << "const double tmp = c[(u64)k * hy_Ns] * cur_h;\nconst double y = tmp - comp;\nconst double t = res + "
                      "y;\n";
                os << "comp = (t - res) - y;\nres = t;\ncur_h = cur_h * h;\n}\n";
                os << "x" << i << " = " << reduced(i, "res") << ";\n}\n";
            }
        } else {
            // Horner (reference: taylor_run_multihorner(), src/taylor_00.cpp:279-351).
            for (std::uint32_t i = 0; i < n_eq; ++i) {
                os << "{\nconst double *c = jet + (u64)" << (static_cast<std::uint64_t>(i) * (order + 1u))
                   << "u * hy_Ns;\n";
                os << "double res = c[(u64)" << order << "u * hy_Ns];\n";
                os << "#pragma unroll\nfor (unsigned k = 1; k <= " << order << "u; ++k) {\n";
                os << "res = c[(u64)(" << order << "u - k) * hy_Ns] + res * h;\n}\n";
                os << "x" << i << " = " << reduced(i, "res") << ";\n}\n";
            }
        }

    }

    // ---- Bookkeeping (emit_detail::step_loop_source(), HY_STEP_TAIL). ----
    os << "HY_STEP_ADVANCE\nbool nf = !(hy_finite(t_hi) & hy_finite(t_lo));\n";
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        os << "nf = nf | !hy_finite(x" << i << ");\n";
    }
    os << R"HIP(
HY_STEP_TAIL(nf, true)
}
)HIP";
    if (!p.ev_u.empty() && !reg_jets) {
        os << "if (a.mode == 4) {\na.last_h[s] = last_h;\nreturn;\n}\n";
    }
    for (std::uint32_t i = 0; i < n_eq; ++i) {
        os << "a.state[(u64)" << i << "u * N + s] = x" << i << ";\n";
    }
    os << "HY_STEP_RESULT(s)\n}\n";

    n_stmt += e.n_stmt;
    return os.str();
}

// Estimate (in doubles) of what a lane must keep alive in register-jet mode: the jets of the state variables
// that are neither constant nor defined by another state variable, plus the history of the operands of the
// nonlinear nodes.
std::uint64_t reg_jet_estimate(const taylor_program &p, std::uint32_t order, bool folded = false)
{
    std::uint64_t n = 0;
    for (const auto &d : p.sv_defs) {
        if (d.type == operand::kind::uvar && d.idx >= p.n_eq) {
            n += order + 1u;
        }
    }
    for (const auto h : history_operands(p, folded)) {
        n += (h != 0) ? order : 0u;
    }
    return n;
}

emitted_module emit_unrolled(const taylor_program &p, const emit_options &opts)
{
    std::ostringstream src;
    src << prelude() << step_loop_source() << (opts.angle_reduce.empty() ? "" : angle_reduce_helper_source) << rules_source(p);
    emit_dout(src, p, opts);

    emitted_module ret;
    ret.angle_reduce_fused = !opts.angle_reduce.empty();
    // Register-resident jets when they fit comfortably in the 512 VGPR+AGPR of a lane.
    // NOTE: the stepper with events needs the Taylor coefficients in memory (event detection, dense output).
    // (Round 6: the estimate counts what the generator really keeps when it folds scaled copies and u + number into their
    // parents - default arithmetic only -, and the limit went from 200 to 270 doubles: two massive bodies 226, 1.24e9 -> 8.7e9
    // system-steps/s, cr3bp 265, 3.0e9 -> 6.6e9, both with 10 ... 16 spilled registers of 512 - against jets which travel
    // through HBM at every step; profiles/r06_model_rates.log. HEYOKA_AMD_REG_JETS_MAX overrides the limit.)
    const bool folds = opts.dev.unrolled_trim && !opts.exact_division && opts.sum_order == 0;
    const bool reg_jets
        = p.ev_u.empty()
          && reg_jet_estimate(p, opts.order, folds)
                 <= static_cast<std::uint64_t>(opts.dev.reg_jets_max >= 0 ? opts.dev.reg_jets_max : (folds ? 270 : 200));
    if (reg_jets) {
        // Two wavefronts per SIMD (256 registers per lane) when what a lane keeps through the orders leaves room for the
        // working set: measured on the two-body problem with a test particle, where the histories of the velocities are
        // re-derived (5 histories instead of 8: 1.26e10 -> 1.38e10 system-steps/s with 50 spilled registers; with all 8
        // histories the same attribute costs 2.3x, profiles/r05_ab_two_body_one_vs_two_wavefronts.log). Only there: a
        // decomposition which keeps that little WITHOUT the re-derivation is compiled as before (not measured).
        // HEYOKA_AMD_UNROLLED_WAVES=n forces n.
        int waves = opts.dev.unrolled_waves;
        if (waves == 0) {
            std::uint64_t n_tmp = 0;
            std::uint32_t n_derived = 0;
            emit_unrolled_kernel(p, opts, "hy_taylor", true, n_tmp, false, 0, &n_derived);
            const auto est = reg_jet_estimate(p, opts.order);
            detail::log_message(log_level::debug, "straight-line stepper: " + std::to_string(est) + " doubles kept per lane (estimate), the histories of "
                                                      + std::to_string(n_derived) + " state variables re-derived at the end of the step");
            if (n_derived > 0u && est >= static_cast<std::uint64_t>(n_derived) * (opts.order + 1u)
                && est - static_cast<std::uint64_t>(n_derived) * (opts.order + 1u) <= 126u) {
                waves = 2;
            }
        }
        src << emit_unrolled_kernel(p, opts, "hy_taylor", true, ret.n_statements, false, waves);
        // NOTE: the variant serving write_tc streams the coefficients out of the same register-resident code (round 1
        // went through the jets-in-memory kernel: 512 registers, 790 spilled dwords for the two-body problem).
        src << emit_unrolled_kernel(p, opts, "hy_taylor_tc", true, ret.n_statements, true, waves);
        ret.tc_kernel_name = "hy_taylor_tc";
        ret.tc_optional = true;
        ret.notes = "register-resident state jets (+ variant streaming the Taylor coefficients out)";
        if (waves == 2 && opts.dev.unrolled_waves == 0) {
            ret.notes += ", two wavefronts per SIMD (coefficient histories of the variables which only define x' = v re-derived)";
        }
    } else {
        src << emit_unrolled_kernel(p, opts, "hy_taylor", false, ret.n_statements, false, opts.dev.unrolled_waves);
    }
    ret.source = src.str();
    ret.kernel_name = "hy_taylor";
    ret.dout_name = "hy_dout";
    ret.block_size = opts.block_size;
    ret.lanes_per_system = 1;
    ret.mode = emit_mode::unrolled;
    return ret;
}

} // namespace emit_detail

dev_switches dev_switches::from_env()
{
    dev_switches d;
    const auto off = [](const char *name) {
        const char *e = std::getenv(name);
        return e != nullptr && std::atoi(e) == 0;
    };
    const auto set = [](const char *name) { return std::getenv(name) != nullptr; };
    const auto num = [](const char *name, int dflt) {
        const char *e = std::getenv(name);
        return e != nullptr ? std::atoi(e) : dflt;
    };
    const auto str = [](const char *name) {
        const char *e = std::getenv(name);
        return e != nullptr ? std::string(e) : std::string{};
    };
    d.v5_events = !off("HEYOKA_AMD_V5_EVENTS");
    d.compact_tc = !off("HEYOKA_AMD_COMPACT_TC");
    d.events_in_stepper = !set("HEYOKA_AMD_NO_EVENTS_IN_STEPPER");
    d.pair_events = !set("HEYOKA_AMD_NO_PAIR_EVENTS");
    d.refill = !set("HEYOKA_AMD_NO_REFILL");
    d.block_v2 = !off("HEYOKA_AMD_BLOCK_V2");
    d.state_aliases = !set("HEYOKA_AMD_NO_STATE_ALIASES");
    d.cluster_v1 = set("HEYOKA_AMD_CLUSTER_V1");
    d.multi_class = !(std::getenv("HEYOKA_AMD_MULTI_CLASS") != nullptr && std::string(std::getenv("HEYOKA_AMD_MULTI_CLASS")) == "0");
    d.linearise = !set("HEYOKA_AMD_NO_LINEARISED_SUMS");
    d.table_lds = num("HEYOKA_AMD_TABLE_LDS", -1);
    d.staged_wps = num("HEYOKA_AMD_STAGED_WPS", 0);
    d.ev_inline_max_nonlinear = num("HEYOKA_AMD_EV_INLINE_MAX_NONLINEAR", -1);
    d.v5_prio = num("HEYOKA_AMD_V5_PRIO", 2);
    d.unrolled_waves = num("HEYOKA_AMD_UNROLLED_WAVES", 0);
    d.unrolled_trim = !off("HEYOKA_AMD_UNROLLED_TRIM");
    d.unrolled_merge_ssq = !off("HEYOKA_AMD_UNROLLED_MERGE_SSQ");
    d.unrolled_derive = !off("HEYOKA_AMD_UNROLLED_DERIVE");
    d.reg_jets_max = num("HEYOKA_AMD_REG_JETS_MAX", -1);
    d.v5_opts = str("HEYOKA_AMD_V5_OPTS");
    d.v5_pad = str("HEYOKA_AMD_V5_PAD");
    d.block_opts = str("HEYOKA_AMD_BLOCK_OPTS");
    return d;
}

} // namespace heyoka_amd
