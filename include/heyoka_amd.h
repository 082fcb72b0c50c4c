/*
 * heyoka_amd C ABI: the drop-in boundary of the MI355X batch Taylor integrator.
 *
 * Every entry point replaces (and is named after) a piece of the public C++ interface of
 * bluescarni/heyoka v7.12.0 on the taylor_adaptive_batch<double> / ensemble_propagate_* path; the
 * reference interface each one stands for is cited as file:line relative to the reference tree.
 * Plain pointers and sizes only: no C++ or torch types cross this boundary.
 *
 * Conventions
 *  - All per-system arrays use the reference's batch layout array[row * batch_size + lane]
 *    (src/taylor_adaptive_batch.cpp:679, src/taylor_00.cpp:574-575, :835).
 *  - Functions returning int return 0 on success, otherwise one of the HY_ERR_* codes; the message
 *    (identical to the exception message of the reference where one exists) is available from
 *    hy_last_error() on the calling thread.
 *  - Functions returning a handle return NULL on error.
 *  - Pointers named d_* are device (HBM) pointers; everything else is host memory.
 */
#ifndef HEYOKA_AMD_H
#define HEYOKA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HY_OK 0
#define HY_ERR_INVALID_ARGUMENT 1 /* std::invalid_argument in the reference */
#define HY_ERR_OVERFLOW 2         /* std::overflow_error */
#define HY_ERR_NOT_IMPLEMENTED 3  /* heyoka::not_implemented_error (include/heyoka/exceptions.hpp) */
#define HY_ERR_RUNTIME 4          /* std::runtime_error / HIP / hiprtc failures */

/* taylor_outcome (include/heyoka/taylor.hpp:142-155). */
#define HY_OUTCOME_SUCCESS (-4294967296LL - 1)
#define HY_OUTCOME_STEP_LIMIT (-4294967296LL - 2)
#define HY_OUTCOME_TIME_LIMIT (-4294967296LL - 3)
#define HY_OUTCOME_ERR_NF_STATE (-4294967296LL - 4)
#define HY_OUTCOME_CB_STOP (-4294967296LL - 5)

const char *hy_last_error(void);
/* HY_ERR_* code of the last failed call on the calling thread (for functions returning handles). */
int hy_last_error_code(void);
void hy_free_str(char *);
/* Library/toolchain information: "heyoka_amd <version>; gfx950; hiprtc <ver>". Caller frees. */
char *hy_version(void);
/* Build id of the library: the first 16 hex digits of the SHA-256 over its sources (the .cpp and .hpp files of heyoka_amd/csrc in sorted
 * order, then this header). The Python host layer recomputes it from the tree at import and refuses a library which does
 * not match (a stale prebuilt .so); bench.py prints it next to the sha of the generated kernel. Static string. */
const char *hy_build_id(void);
/* Stage logger (include/heyoka/logging.hpp:19-24: set_logger_level_trace() ... _critical(); src/logging.cpp:20-48): level
 * 0 trace, 1 debug, 2 info, 3 warn (default), 4 err, 5 critical, 6 off. Logged at construction: the size of the Taylor
 * decomposition (debug), the generator the planner chose with the reasons the others did not apply (info; warn when a large
 * decomposition falls to a generic stepper), and the decomposition / code generation / hiprtc times (trace). Messages go to
 * stderr unless a callback is installed. */
typedef void (*hy_log_callback_t)(int level, const char *msg, void *user);
int hy_set_logger_level(int level);
int hy_get_logger_level(void);
void hy_set_log_callback(hy_log_callback_t cb, void *user);
/* Number of visible HIP devices (0 without a GPU). */
int hy_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Expressions (include/heyoka/expression.hpp:73-118; operators src/expression_ops.cpp:34-91).
 * Handles are owned by the caller and released with hy_expr_free(). Functions never consume
 * their arguments.
 * --------------------------------------------------------------------------------------------- */
typedef struct hy_expr_s *hy_expr;

hy_expr hy_expr_var(const char *name);    /* expression{variable{name}}   expression.hpp:73 */
hy_expr hy_expr_num(double value);        /* expression{number{value}}    number.hpp */
hy_expr hy_expr_par(uint32_t index);      /* par[index]                   param.hpp */
hy_expr hy_expr_time(void);               /* heyoka::time                 math/time.hpp */
hy_expr hy_expr_neg(hy_expr);             /* operator-(e)                 expression_ops.cpp:45-52 */
hy_expr hy_expr_add(hy_expr, hy_expr);    /* operator+                    expression_ops.cpp:55-62 */
hy_expr hy_expr_sub(hy_expr, hy_expr);    /* operator-                    expression_ops.cpp:65-72 */
hy_expr hy_expr_mul(hy_expr, hy_expr);    /* operator*                    expression_ops.cpp:75-82 */
hy_expr hy_expr_div(hy_expr, hy_expr);    /* operator/                    expression_ops.cpp:85-91 */
hy_expr hy_expr_pow(hy_expr, hy_expr);    /* pow()                        src/math/pow.cpp:1066 */
hy_expr hy_expr_sqrt(hy_expr);            /* sqrt()                       src/math/sqrt.cpp:16 */
hy_expr hy_expr_sin(hy_expr);             /* sin()                        src/math/sin.cpp:406 */
hy_expr hy_expr_cos(hy_expr);             /* cos()                        src/math/cos.cpp:406 */
hy_expr hy_expr_exp(hy_expr);             /* exp()                        src/math/exp.cpp */
hy_expr hy_expr_log(hy_expr);             /* log()                        src/math/log.cpp */
/* Elementary functions beyond the N-body set (include/heyoka/math/{tan,tanh,sinh,cosh,asin,acos,atan,asinh,
 * acosh,atanh,erf,sigmoid}.hpp; Taylor rules src/math/<name>.cpp). */
hy_expr hy_expr_tan(hy_expr);
hy_expr hy_expr_tanh(hy_expr);
hy_expr hy_expr_sinh(hy_expr);
hy_expr hy_expr_cosh(hy_expr);
hy_expr hy_expr_asin(hy_expr);
hy_expr hy_expr_acos(hy_expr);
hy_expr hy_expr_atan(hy_expr);
hy_expr hy_expr_asinh(hy_expr);
hy_expr hy_expr_acosh(hy_expr);
hy_expr hy_expr_atanh(hy_expr);
hy_expr hy_expr_erf(hy_expr);
hy_expr hy_expr_sigmoid(hy_expr);
hy_expr hy_expr_atan2(hy_expr y, hy_expr x); /* atan2(y, x)                  src/math/atan2.cpp:763 */
hy_expr hy_expr_kepE(hy_expr e, hy_expr M);  /* eccentric anomaly E(e, M)    src/math/kepE.cpp:801 */
/* Piecewise functions: relu / relup with the slope of the leaky variants (src/math/relu.cpp:580-602), select(c, t, f)
 * (src/math/select.cpp:267), logical_and (is_and != 0) / logical_or (src/math/logical.cpp:314-338), comparisons
 * op = 0..5 -> eq, neq, lt, gt, lte, gte (src/math/relational.cpp:343-354). */
hy_expr hy_expr_relu(hy_expr x, double slope);
hy_expr hy_expr_relup(hy_expr x, double slope);
hy_expr hy_expr_select(hy_expr cond, hy_expr t, hy_expr f);
hy_expr hy_expr_logical(int is_and, const hy_expr *args, size_t n);
hy_expr hy_expr_rel(int op, hy_expr a, hy_expr b);
/* ---- Node rules: the per-function extension seam (reference: func_base, include/heyoka/func.hpp:94-96, :117-147; a
 * function without a Taylor rule raises not_implemented_error, func.hpp:266-267 -> HY_ERR_NOT_IMPLEMENTED here).
 * A rule is the counterpart of a func_base subclass (heyoka_amd/csrc/node_rule.hpp):
 *   - decompose(): fills hidden_out[0 .. n_hidden) with the definitions of the hidden u variables appended behind the node
 *     (what a taylor_decompose() override appends by hand); each is ONE elementary function of `self` (the node), its
 *     arguments and hidden_vars[j], j < own index. Returns 0 on success. The callee owns nothing: every handle it
 *     creates and stores in hidden_out is released by the library.
 *   - hidden_deps[4 * j .. 4 * j + 4): the hidden dependencies of hidden definition j (indices into the hidden
 *     definitions, -1 = none), e.g. sin(self) <-> cos(self);
 *   - deps[0 .. n_deps): the hidden dependencies of the node itself, in the order hy_rule_<name>_orderk() reads them;
 *   - hip_source: HIP device code defining
 *         double hy_rule_<name>_order0(const double *x);
 *         double hy_rule_<name>_orderk(unsigned k, const hy_jet &a, const hy_jet *x, const hy_jet *h);
 *     (the taylor_diff() / taylor_c_diff_func() pair of the reference: one text serves the straight-line generator, the
 *     interpreted steppers and compiled functions). */
typedef int (*hy_node_rule_decompose_fn)(void *ctx, hy_expr self, const hy_expr *args, uint32_t n_args,
                                         const hy_expr *hidden_vars, hy_expr *hidden_out);
typedef struct hy_node_rule_desc {
    const char *name;
    uint32_t n_args;
    uint32_t n_hidden;
    hy_node_rule_decompose_fn decompose; /* NULL iff n_hidden == 0 */
    void *ctx;
    const int32_t *hidden_deps; /* 4 * n_hidden entries, may be NULL if no hidden definition has dependencies */
    const uint32_t *deps;
    uint32_t n_deps;
    const char *hip_source;
} hy_node_rule_desc;
int hy_node_rule_register(const hy_node_rule_desc *); /* HY_OK / HY_ERR_INVALID_ARGUMENT (duplicate, malformed) */
/* f(args) of a registered rule; NULL + HY_ERR_NOT_IMPLEMENTED for an unknown name. */
hy_expr hy_expr_custom(const char *name, const hy_expr *args, size_t n);
/* Defined through the registry alone (csrc/builtin_rules.cpp): kepF(h, k, lam), F + h cos F - k sin F = lam
 * (src/math/kepF.cpp:1689), and kepDE(s0, c0, DM), DE - c0 sin DE + s0 (1 - cos DE) = DM (src/math/kepDE.cpp:113). */
hy_expr hy_expr_kepF(hy_expr h, hy_expr k, hy_expr lam);
hy_expr hy_expr_kepDE(hy_expr s0, hy_expr c0, hy_expr DM);
/* heyoka::pi: a constant which is a function without arguments with its own u variable (include/heyoka/math/constants.hpp:117,
 * src/math/constants.cpp:258-273); a registered rule as well. */
hy_expr hy_expr_pi(void);
hy_expr hy_expr_sum(const hy_expr *, size_t n);  /* sum(vector)           src/math/sum.cpp:548 */
hy_expr hy_expr_prod(const hy_expr *, size_t n); /* prod(vector)          src/math/prod.cpp:913 */
void hy_expr_free(hy_expr);
char *hy_expr_str(hy_expr); /* caller frees with hy_free_str() */
/* diff(e, x) (include/heyoka/expression.hpp, diff(const expression &, const expression &)): x a variable or par[i]. One rule
 * per built-in function, memoised on shared nodes, zeros and ones folded by the operators; a function defined through a
 * node rule (kepF, kepDE, hy_expr_custom) has no gradient: NULL + HY_ERR_NOT_IMPLEMENTED naming it. */
hy_expr hy_expr_diff(hy_expr e, hy_expr x);
/* Value of e on the HOST (libm; Newton iteration for kepE): variables names[i] = values[i], par[i] = pars[i], heyoka::time =
 * time. HY_ERR_INVALID_ARGUMENT for a variable or parameter without a value, HY_ERR_NOT_IMPLEMENTED for a node-rule function. */
int hy_expr_eval(hy_expr e, const char *const *names, const double *values, size_t n_vars, const double *pars, size_t n_pars,
                 double time, double *out);
/* Number of distinct function nodes (shared nodes counted once) below the n expressions: the size of their DAG. */
size_t hy_expr_node_count(const hy_expr *, size_t n);

/* ------------------------------------------------------------------------------------------------
 * ODE systems: std::vector<std::pair<expression, expression>> (prime(x) = rhs).
 * --------------------------------------------------------------------------------------------- */
typedef struct hy_sys_s *hy_sys;

hy_sys hy_sys_new(void);
int hy_sys_add(hy_sys, hy_expr lhs, hy_expr rhs); /* prime(lhs) = rhs */
size_t hy_sys_size(hy_sys);
void hy_sys_free(hy_sys);
/* model::nbody(n, kw::masses, kw::Gconst) (include/heyoka/model/nbody.hpp:73-78, src/model/nbody.cpp:53-174).
 * masses == NULL -> all masses equal to 1 (n_masses ignored). */
hy_sys hy_model_nbody(uint32_t n, const double *masses, size_t n_masses, double Gconst);
/* model::pendulum(kw::gconst, kw::length) (src/model/pendulum.cpp:23-28). */
hy_sys hy_model_pendulum(double gconst, double length);
/* General form of model::nbody(): masses and Gconst as expressions (numbers or par[i]; runtime parameters
 * select the non-grouped branch src/model/nbody.cpp:131-150). masses == NULL -> all 1; Gconst == NULL -> 1. */
hy_sys hy_model_nbody_ex(uint32_t n, const hy_expr *masses, size_t n_masses, hy_expr Gconst);
/* model::nbody_energy() / nbody_potential() (include/heyoka/model/nbody.hpp:80-92, src/model/nbody.cpp:176-235),
 * model::pendulum_energy() (src/model/pendulum.cpp:31-36): expressions of the state variables
 * x_i, y_i, z_i, vx_i, vy_i, vz_i (resp. x, v), ready for hy_cfunc_new(). */
hy_expr hy_model_nbody_energy(uint32_t n, const hy_expr *masses, size_t n_masses, hy_expr Gconst);
hy_expr hy_model_nbody_potential(uint32_t n, const hy_expr *masses, size_t n_masses, hy_expr Gconst);
hy_expr hy_model_pendulum_energy(double gconst, double length);
/* The other point-mass models. Expression arguments are numbers or par[i]; a NULL
 * Gconst / mu selects the reference's default (1 resp. 1e-3), an empty omega a non-rotating frame.
 *   model::np1body / np1body_energy / np1body_potential  include/heyoka/model/nbody.hpp:94-120, src/model/nbody.cpp:236-445
 *   model::cr3bp / cr3bp_jacobi                          include/heyoka/model/cr3bp.hpp:30-64, src/model/cr3bp.cpp
 *   model::fixed_centres{,_energy,_potential}            include/heyoka/model/fixed_centres.hpp, src/model/fixed_centres.cpp
 *   model::rotating{,_energy,_potential}                 include/heyoka/model/rotating.hpp, src/model/rotating.cpp
 *   model::mascon{,_energy,_potential}                   include/heyoka/model/mascon.hpp, src/model/mascon.cpp
 * State variables: x_i, y_i, z_i, vx_i, vy_i, vz_i (i = 1..n-1) for np1body; x, y, z, px, py, pz for cr3bp;
 * x, y, z, vx, vy, vz for the others. positions holds 3 entries per mass. */
hy_sys hy_model_np1body(uint32_t n, const hy_expr *masses, size_t n_masses, hy_expr Gconst);
hy_expr hy_model_np1body_energy(uint32_t n, const hy_expr *masses, size_t n_masses, hy_expr Gconst);
hy_expr hy_model_np1body_potential(uint32_t n, const hy_expr *masses, size_t n_masses, hy_expr Gconst);
hy_sys hy_model_cr3bp(hy_expr mu);
hy_expr hy_model_cr3bp_jacobi(hy_expr mu);
hy_sys hy_model_fixed_centres(hy_expr Gconst, const hy_expr *masses, size_t n_masses, const hy_expr *positions,
                              size_t n_positions);
hy_expr hy_model_fixed_centres_energy(hy_expr Gconst, const hy_expr *masses, size_t n_masses, const hy_expr *positions,
                                      size_t n_positions);
hy_expr hy_model_fixed_centres_potential(hy_expr Gconst, const hy_expr *masses, size_t n_masses,
                                         const hy_expr *positions, size_t n_positions);
hy_sys hy_model_rotating(const hy_expr *omega, size_t n_omega);
hy_expr hy_model_rotating_energy(const hy_expr *omega, size_t n_omega);
hy_expr hy_model_rotating_potential(const hy_expr *omega, size_t n_omega);
hy_sys hy_model_mascon(hy_expr Gconst, const hy_expr *masses, size_t n_masses, const hy_expr *positions,
                       size_t n_positions, const hy_expr *omega, size_t n_omega);
hy_expr hy_model_mascon_energy(hy_expr Gconst, const hy_expr *masses, size_t n_masses, const hy_expr *positions,
                               size_t n_positions, const hy_expr *omega, size_t n_omega);
hy_expr hy_model_mascon_potential(hy_expr Gconst, const hy_expr *masses, size_t n_masses, const hy_expr *positions,
                                  size_t n_positions, const hy_expr *omega, size_t n_omega);
/* The state variables of a system, in order (the lhs of each equation); out[hy_sys_size()] receives new
 * handles owned by the caller. */
int hy_sys_get_vars(hy_sys, hy_expr *out);
/* The right-hand sides, in the same order and under the same ownership rule. */
int hy_sys_get_rhs(hy_sys, hy_expr *out);
/* taylor_decompose_sys() (src/taylor_01.cpp:848-1008): one line per entry of the decomposition,
 * "u_i = ..." textual form with hidden dependencies. Caller frees with hy_free_str(). */
char *hy_sys_decomposition_str(hy_sys);

/* ------------------------------------------------------------------------------------------------
 * var_ode_sys (include/heyoka/var_ode_sys.hpp:29-75, src/var_ode_sys.cpp:215-407): the system augmented with the
 * equations of the derivatives of the state with respect to initial conditions and parameters, up to `order` >= 1.
 * var_args_mask != 0: the var_args enumerator (1 vars, 2 params, 1|2 both); 0: the explicit list args[0..n_args) of state
 * variables and par[i]. Time as an argument (mask bit 4, hy_expr_time()) is not implemented: HY_ERR_NOT_IMPLEMENTED.
 * Equations: the original ones first, then one variable per (component, multi-index), sorted by total order, component,
 * reverse-lexicographic multi-index, named "\xe2\x88\x82" + sparse index list + name as in the reference.
 * --------------------------------------------------------------------------------------------- */
typedef struct hy_var_sys_s *hy_var_sys;
hy_var_sys hy_var_sys_new(hy_sys sys, int var_args_mask, const hy_expr *args, size_t n_args, uint32_t order);
void hy_var_sys_free(hy_var_sys);
hy_sys hy_var_sys_get_sys(hy_var_sys);           /* get_sys(): a new handle, hy_sys_free() */
uint32_t hy_var_sys_get_n_orig_sv(hy_var_sys);   /* get_n_orig_sv() */
uint32_t hy_var_sys_get_order(hy_var_sys);       /* get_order() */
size_t hy_var_sys_get_n_vargs(hy_var_sys);
int hy_var_sys_get_vargs(hy_var_sys, hy_expr *out); /* get_vargs(): new handles */
/* get_didx_range() in dense form: components[e] and multi_indices[e * n_vargs + a] for every equation e of get_sys(). */
int hy_var_sys_get_didx(hy_var_sys, uint32_t *components, uint32_t *multi_indices);

/* ------------------------------------------------------------------------------------------------
 * taylor_adaptive_batch<double> (include/heyoka/taylor.hpp:781-1121).
 * --------------------------------------------------------------------------------------------- */
typedef struct hy_tab_s *hy_tab;

/* Keyword arguments of the constructor (taylor.hpp:814-821, :905-941). */
typedef struct {
    double tol;            /* kw::tol; 0 -> default (machine epsilon) */
    int high_accuracy;     /* kw::high_accuracy */
    int compact_mode;      /* kw::compact_mode (accepted; code generation mode is chosen internally) */
    int parallel_mode;     /* kw::parallel_mode (validated like the reference, otherwise ignored) */
    const double *pars;    /* kw::pars, n_pars values (NULL -> zeros) */
    size_t n_pars;
    const double *time;    /* kw::time: NULL -> 0; n_time == 1 -> scalar splat; else batch_size values */
    size_t n_time;
    int device;            /* HIP device ordinal (MI355X extension) */
    /* MI355X extensions; 0 = default everywhere (a zero-initialised structure behaves like the reference). */
    int emitter;           /* code generator: 0 automatic, 1 unrolled, 2 wave-cluster, 3 table (the compact-mode analogue), 4 block */
    int cluster_kernel;    /* wave-cluster generator: 0 automatic, 5 one lane per pair, 3 lane pairs, 2 pipelined, 1 first generation */
    int exact_division;    /* != 0: correctly rounded quotients in the recurrences of the pair kernels (default: reciprocal forms, within 1 ulp) */
    int events_on_cluster; /* 0 automatic; 1: integrators with events always use the one-system-per-lane steppers */
    int sum_order;         /* additions inside the convolutions of the unrolled generator: 0 automatic (= 2), 1 the reference's
                            * default mode (products first, pairwise sum), 2 its compact mode (running sums: one FMA per term) */
    int batch_semantics;   /* propagate_for/until when a lane goes non-finite or max_steps is hit: 0 the reference's batch-wide
                            * outcomes (src/taylor_adaptive_batch.cpp:1404-1407, :1462-1467, :1516), 1 always the lock-step loop,
                            * 2 per-lane outcomes of the device-resident path (no snapshot, fully asynchronous),
                            * 3 independent: as 2, and within one propagate_until / propagate_for / propagate_grid call a system
                            * whose step ends in a stopping terminal event (outcome -index - 1) or in a non-finite state is retired
                            * alone - it keeps the state, time and outcome of that step and takes zero-length steps from then on -
                            * while every other system carries on to its final time (hy_tab_get_n_retired()) */
} hy_tab_config;

/* Constructor (taylor.hpp:905-941 -> finalise_ctor_impl(), src/taylor_adaptive_batch.cpp:78-427).
 * state: n_state = n_eq * batch_size values, or n_state == 0 for a zero-initialised state.
 * Performs decomposition, HIP code generation and hiprtc compilation; does not need a GPU. */
hy_tab hy_tab_create(hy_sys sys, const double *state, size_t n_state, uint32_t batch_size, const hy_tab_config *cfg);
/* Event detection (kw::t_events / kw::nt_events, include/heyoka/events.hpp:52-325; detection
 * src/detail/event_detection.cpp:1733-2173; event branch of step_impl() src/taylor_adaptive_batch.cpp:727-1030).
 * direction: -1 negative, 0 any, +1 positive (event_direction). Callbacks run on the host, one lane at a time:
 *   non-terminal: cb(integrator, trigger time, sign of d(eq)/dt, batch index, user)
 *   terminal:     cb(...) returns non-zero to continue, zero to stop the propagation; cb == NULL always stops.
 *   cooldown < 0 -> deduced automatically (taylor_deduce_cooldown()).
 * Outcomes follow the reference: step outcome = event index (continuing) or -index - 1 (stopping). */
typedef void (*hy_nt_event_cb)(hy_tab, double time, int d_sgn, uint32_t batch_idx, void *user);
typedef int (*hy_t_event_cb)(hy_tab, int d_sgn, uint32_t batch_idx, void *user);
typedef struct {
    hy_expr eq;
    hy_nt_event_cb cb;
    void *user;
    int direction;
} hy_nt_event;
typedef struct {
    hy_expr eq;
    hy_t_event_cb cb;
    void *user;
    int direction;
    double cooldown;
} hy_t_event;
hy_tab hy_tab_create_with_events(hy_sys sys, const double *state, size_t n_state, uint32_t batch_size,
                                 const hy_tab_config *cfg, const hy_t_event *t_events, size_t n_t_events,
                                 const hy_nt_event *nt_events, size_t n_nt_events);
int hy_tab_with_events(hy_tab);
/* The constructor over a variational system. n_state = (number of equations) * batch_size, or n_orig_sv * batch_size (or 0):
 * the variational variables then start from 1 where a first-order derivative is taken with respect to its own state variable
 * and from 0 elsewhere (src/detail/setup_variational_ics.cpp:49-121). Everything else - events, callbacks, grids, batch
 * semantics - sees a system of hy_tab_get_dim() equations. The module of the Taylor map is compiled here as well. */
hy_tab hy_tab_create_var(hy_var_sys vsys, const double *state, size_t n_state, uint32_t batch_size, const hy_tab_config *cfg,
                         const hy_t_event *t_events, size_t n_t_events, const hy_nt_event *nt_events, size_t n_nt_events);
int hy_tab_is_variational(hy_tab);          /* is_variational() */
uint32_t hy_tab_get_n_orig_sv(hy_tab);      /* get_n_orig_sv(): the dimension for a non-variational integrator */
/* get_vorder() / get_vargs(): HY_ERR_INVALID_ARGUMENT with the reference's message on a non-variational integrator. */
int hy_tab_get_vorder(hy_tab, uint32_t *order);
int hy_tab_get_n_vargs(hy_tab, size_t *n);
int hy_tab_get_vargs(hy_tab, hy_expr *out);
/* eval_taylor_map(in) (src/taylor_adaptive_batch.cpp:2415-2470): in[a * batch_size + sys], n = n_vargs * batch_size values
 * (the reference's messages for other sizes); out (may be NULL) and hy_tab_get_tstate() receive out[i * batch_size + sys],
 * i < n_orig_sv. One launch of the kernel hy_tmap over the device-resident state:
 *     out_i = sum_alpha state_(i,alpha) * RN(1 / alpha!) * in^alpha,
 * terms in equation order from the order-0 term, accumulated with fma, monomials by the graded schedule
 * in^alpha = in^(alpha - e_j) * in_j with j the highest non-zero index of alpha. */
int hy_tab_eval_taylor_map(hy_tab, const double *in, size_t n, double *out);
int hy_tab_get_tstate(hy_tab, double *out);  /* get_tstate(): n_orig_sv * batch_size */
/* MI355X extensions. The same evaluation on device buffers, asynchronous on the integrator's stream (get_tstate() is not
 * touched); and the cloud form, kernel hy_tmap_cloud: n_samples displacement vectors per system in sample-fastest layouts,
 * d_delta[(sys * n_vargs + a) * n_samples + m] - or ONE cloud for all systems, d_delta[a * n_samples + m], when shared_cloud
 * != 0 - and d_out[(sys * n_orig_sv + i) * n_samples + m]. Every sample gets the bits hy_tab_eval_taylor_map() gives for
 * the same displacement. The buffers are the caller's: d_in n_vargs * batch_size doubles, d_out n_orig_sv * batch_size; for
 * the cloud d_delta (shared_cloud ? 1 : batch_size) * n_vargs * n_samples and d_out batch_size * n_orig_sv * n_samples.
 * HY_ERR_NOT_IMPLEMENTED (every evaluation of the map and hy_tab_taylor_map_module()) when the integrator has no map: no
 * variational arguments, or the coefficients of ONE output beyond the 64 KiB of LDS a workgroup can declare. */
int hy_tab_eval_taylor_map_device(hy_tab, const double *d_in, double *d_out);
int hy_tab_eval_taylor_map_cloud(hy_tab, const double *d_delta, double *d_out, uint64_t n_samples, int shared_cloud);
/* Introspection hook (test suite): HIP source (hy_free_str()) and gfx950 code object (owned by the integrator) of the
 * Taylor-map module of a variational integrator. Either output may be NULL. */
int hy_tab_taylor_map_module(hy_tab, char **source, const char **data, size_t *size);
/* The source of the module for (n_orig_sv, n_args, order) without an integrator. lds_bytes: LDS the cloud kernel may use per
 * workgroup for coefficients (0: the default, 16 KiB) - beyond it the outputs are processed in groups; *note (may be NULL,
 * hy_free_str()) receives the stage logger's line about the decision. */
char *hy_taylor_map_source(uint32_t n_orig_sv, uint32_t n_args, uint32_t order, size_t lds_bytes, char **note);
/* Accounting of the steps with events (bench.py's events leg). out8 = {steps with events, ms upload / buffers, ms stepper
 * (+ event jets), ms detection kernel, ms bookkeeping kernel + flags to the host, ms state update + records, regeneration
 * launches of the Taylor coefficients, systems which reported events}; the five phase times accumulate only while the
 * timing is on (hy_tab_set_event_timing(): one stream synchronisation per phase). */
int hy_tab_set_event_timing(hy_tab, int on);
int hy_tab_get_event_stats(hy_tab, double *out8);
/* batch_semantics = 3: systems retired (stopping terminal event or non-finite state) by the last propagate_until / propagate_for /
 * propagate_grid call which went through the sweep loop; 0 under the other semantics. */
uint64_t hy_tab_get_n_retired(hy_tab);
/* != 0: every event of the integrator is applied on the device (library-side counting / recording callbacks and, under
 * batch_semantics = 3, terminal events without a callback): no records, no per-event host work. Needs no GPU. */
int hy_tab_events_on_device(hy_tab);
/* Ready-made callbacks which count their invocations in the uint64_t `user` points to (the terminal one continues).
 * When EVERY event of an integrator has one of them as its callback, the step applies the events on the device (counts per
 * event, cooldown and "continuing" outcome of the first terminal event of a lane: what the host loop of
 * src/taylor_adaptive_batch.cpp:837-1030 does) and adds the counts to the counters once per step: no per-event host work. */
void hy_event_counter_nt(hy_tab, double time, int d_sgn, uint32_t batch_idx, void *user);
int hy_event_counter_t(hy_tab, int d_sgn, uint32_t batch_idx, void *user);
/* Ready-made callbacks which RECORD: every invocation appends a row to the integrator's event log and lets the integration
 * continue. `user` may be NULL or point to a uint64_t which is incremented like a counter's. Events with a counter or a
 * callback of the caller's produce no rows. When every event of an integrator has a counting or a recording callback the
 * rows are written on the device (no per-event host work); mixed with other callbacks they are collected by the host loop -
 * the same rows in the same order.
 * A row is 8 + dim doubles (8 with the states switched off), integers stored as doubles:
 *   0 system (batch index), 1 class (0 terminal, 1 non-terminal), 2 event index within its class, 3 d_sgn,
 *   4, 5 trigger time (hi, lo) = new time - h + root in double-length arithmetic (hi is the time a host callback receives),
 *   6 root (offset from the beginning of the step), 7 |d eq/dt| at the root,
 *   8 ... the state at the trigger time (non-terminal: dense output of the step's Taylor coefficients at the root;
 *         terminal: the state after the step, which was truncated at the event).
 * Order: the order in which the host loop would have invoked the callbacks - steps in order; within a step by batch index;
 * within a lane the non-terminal events triggering before the lane's first terminal event by ascending |root| (stable in
 * detection order), then that terminal event. Lanes which went non-finite produce no rows.
 * Recorders next to callbacks of the caller's (host-loop path): the state columns are filled when all the callbacks of the
 * step have run - a callback which changes the state or asks for other Taylor coefficients through the integrator is
 * visible in the rows of that step.
 * The log belongs to the integrator and persists across step / propagate calls; hy_tab_copy() gives the copy an empty log;
 * an integrator without recording callbacks has a log of size 0 and allocates nothing. */
void hy_event_recorder_nt(hy_tab, double time, int d_sgn, uint32_t batch_idx, void *user);
int hy_event_recorder_t(hy_tab, int d_sgn, uint32_t batch_idx, void *user);
uint64_t hy_tab_event_log_size(hy_tab);            /* rows */
uint32_t hy_tab_event_log_row_doubles(hy_tab);     /* doubles per row */
uint64_t hy_tab_event_log_capacity(hy_tab);        /* rows the device buffer holds before it grows (geometrically) */
int hy_tab_get_event_log(hy_tab, uint64_t first, uint64_t count, double *out);
/* Zero-copy: device pointer to the rows (NULL if the log is empty), valid until the next call which steps or clears. */
int hy_tab_event_log_device(hy_tab, const double **rows, uint64_t *n_rows, uint32_t *row_doubles);
int hy_tab_clear_event_log(hy_tab);
int hy_tab_event_log_reserve(hy_tab, uint64_t rows);
/* State columns on (default) / off: rows of 8 doubles, no dense output. Only while the log is empty (error otherwise). */
int hy_tab_set_event_log_states(hy_tab, int on);
int hy_tab_get_event_log_states(hy_tab);
/* Introspection hooks (used by the test suite; not needed to use the log): capacity of the device buffer above, and
 * the two functions below.
 * Code objects (gfx950) of the event-log kernels of an integrator with recording callbacks: which = 0 row headers
 * (hy_evr_count / hy_evr_scan / hy_evr_write), 1 dense output over the rows (hy_dout_rows). Owned by the integrator. */
int hy_tab_event_log_code_object(hy_tab, int which, const char **data, size_t *size);
/* Event-log OBSERVABLES (MI355X extension): n expressions over the state variables, par[...] and the time. While the list
 * is set a row of the log is 8 + n doubles: the header above, then column 8 + k = observable k at the trigger - bit for bit
 * what a compiled function of the same expressions returns for the state columns the same run logs without the list, the
 * parameters of the row's system and time = column 4. The kernel hy_obs_rows (code object: which = 2 above) samples only the
 * state rows the expressions read. The list can be set or cleared (obs == NULL, n == 0) only while the log is empty; the state-column
 * switch keeps its value and has no effect while a list is set; copies of the integrator keep the list. Errors: no recording
 * callbacks, a non-empty log, a variable which is not a state variable, a par[i] beyond the parameters of the integrator.
 * HEYOKA_AMD_EVENT_OBS=registers|staged overrides how the kernel holds the samples (default: registers up to 64 rows read). */
int hy_tab_set_event_log_observables(hy_tab, const hy_expr *obs, uint32_t n);
uint32_t hy_tab_get_event_log_n_observables(hy_tab);
/* Observable k as a new expression handle (caller frees); NULL and hy_last_error() when there is none. */
hy_expr hy_tab_get_event_log_observable(hy_tab, uint32_t k);
/* INTERNAL hooks of the test suite: the HIP source (caller frees; NULL and hy_last_error() on error) of the event-log kernel
 * which = 1 (hy_dout_rows) or 2 (hy_obs_rows) of an integrator, and the source of hy_obs_rows for a system and a list of
 * observables without an integrator and without a GPU - compact_tc / exact_division: the layout of the Taylor coefficients
 * and the divisions of the stepper the rows come from (the wave-cluster steppers with events store compact coefficients). */
char *hy_tab_event_log_source(hy_tab, int which);
char *hy_event_observables_source(hy_sys, const hy_expr *obs, uint32_t n, uint32_t order, int high_accuracy, int compact_tc,
                                  int exact_division);
/* Terminal-event ACTIONS: a library-side terminal callback defined by n assignments vars[k] <- rhs[k] (in this order)
 * instead of code of the caller's - a bounce v <- -c v, an impulse v <- v + dv, a wrap of a coordinate. The left-hand
 * sides are distinct state variables of the system; the right-hand sides may read state variables, parameters, the time
 * and numbers, and all of them read the state from BEFORE the action ({x <- v, v <- x} swaps). hy_event_action_new()
 * fails (NULL, hy_last_error()) on an empty list or a left-hand side which is not a variable; the checks against a
 * system (left-hand side not a state variable or repeated, right-hand side using a variable which is not a state variable
 * or a parameter the system does not have) are made by hy_tab_create_with_events().
 * Use: hy_t_event{eq, hy_event_action_t, handle, ...}. The integrator takes a copy of the handle's contents (the handle
 * may be freed right after the construction) and hy_tab_copy() carries it along. The action runs where the reference
 * invokes the terminal callback - the step has been truncated at the event, state and time are those of the trigger
 * time, the cooldown is set -, for the first terminal event of a system in a step only, and the integration continues
 * (outcome = index of the event). It is applied by a generated kernel (hy_ev_action, one lane per system): behind the
 * device-side event handling when every event of the integrator is library-side (counters, recorders, actions; plain
 * stops under batch_semantics 3), at its place in the host loop, one system at a time, otherwise - the same compiled
 * code, the same bits: those of a hy_cfunc of the right-hand sides over the state variables. Results are not checked for
 * finiteness (the next step reports err_nf_state); Taylor coefficients, last_h, the event log and the cooldowns are left
 * alone. Calling hy_event_action_t directly applies the action (which must be one of the integrator's) to the system
 * batch_idx; it returns 1, or 0 on error (hy_last_error()). */
typedef struct hy_event_action_s *hy_event_action;
hy_event_action hy_event_action_new(const hy_expr *vars, const hy_expr *rhs, size_t n);
hy_event_action hy_event_action_clone(hy_event_action);
void hy_event_action_free(hy_event_action);
char *hy_event_action_str(hy_event_action); /* hy_free_str() */
int hy_event_action_t(hy_tab, int d_sgn, uint32_t batch_idx, void *user);
/* Introspection hook (test suite): HIP source (hy_free_str()) and gfx950 code object (owned by the integrator) of the
 * action module of an integrator with actions; error without one. Either output may be NULL. */
int hy_tab_event_action_module(hy_tab, char **source, const char **data, size_t *size);
/* The same for the companion module of a wave-cluster stepper with events (kernels hy_dout_c and hy_tc_expand; hy_ev_jets
 * when the stepper does not evaluate the event equations itself); error for an integrator without one. */
int hy_tab_event_jets_module(hy_tab, char **source, const char **data, size_t *size);
uint32_t hy_tab_n_event_actions(hy_tab);
/* While hy_tab_set_event_timing() is on, every launch of hy_ev_action runs between two HIP events: the sum of the kernel
 * durations (ms) and the number of timed launches since the construction. */
int hy_tab_event_action_kernel_ms(hy_tab, double *ms, uint64_t *launches);
/* HIP source of the event-detection module for (order, number of terminal / non-terminal events); hy_free_str(). */
char *hy_event_detection_source(uint32_t order, uint32_t n_t_events, uint32_t n_nt_events);
/* reset_cooldowns(): batch_idx < 0 -> all the lanes. */
int hy_tab_reset_cooldowns(hy_tab, int64_t batch_idx);
/* get_te_cooldowns(): [batch_size * n_t_events] arrays indexed [lane * n_t_events + event]; active != 0 where a
 * cooldown is in progress, (first, second) = (elapsed, duration). */
int hy_tab_get_te_cooldowns(hy_tab, double *first, double *second, int *active);
hy_tab hy_tab_copy(hy_tab);  /* copy constructor (taylor.hpp:943) */
void hy_tab_free(hy_tab);

/* Getters (taylor.hpp:951-1029). */
uint32_t hy_tab_get_batch_size(hy_tab);
uint32_t hy_tab_get_order(hy_tab);
uint32_t hy_tab_get_dim(hy_tab);
uint32_t hy_tab_get_n_pars(hy_tab);   /* number of runtime parameters per system */
uint32_t hy_tab_get_n_uvars(hy_tab);  /* size of the decomposition minus n_eq */
double hy_tab_get_tol(hy_tab);
int hy_tab_get_high_accuracy(hy_tab);
int hy_tab_get_compact_mode(hy_tab);
/* No reference counterpart: number of (event, lane, step) triples in which the device-side event detection gave up - root
 * isolation beyond 250 working intervals or more isolating intervals than the order, root finder out of iterations: the
 * cases in which the reference's detect_events(), src/detail/event_detection.cpp:2082-2090, :2150-2165, logs a warning and
 * ignores the event for the step. */
unsigned long long hy_tab_get_event_detection_failures(hy_tab);
double hy_tab_get_compile_seconds(hy_tab);
/* No reference counterpart: doubles of global scratch per resident wavefront which the stepper kernel addresses (its jets or
 * its tape, where they do not live on the chip; 0: none). The driver sizes the buffer as launch grid x wavefronts per
 * workgroup x this. */
unsigned long long hy_tab_get_scratch_per_wave(hy_tab);
char *hy_tab_get_hip_source(hy_tab);  /* generated HIP module (cf. llvm_state::get_ir()); caller frees */
char *hy_tab_get_decomposition_str(hy_tab);
/* No reference counterpart: the rewritten INTERNAL program the stepper was generated from when the planner of the
 * wave-cluster kernels changed it (state-variable aliases, padded clusters, restored unit scalings; the decomposition the
 * user sees is never touched) - one node per line in the format of hy_tab_get_decomposition_str(), then the definitions
 * of the state derivatives; an empty string otherwise. For tests: the rewrites must not change the jets. Caller frees. */
char *hy_tab_get_internal_program(hy_tab);
/* Description of the code generation mode chosen for this system ("unrolled", "cluster ...", "table ..."). Caller frees. */
char *hy_tab_get_codegen_info(hy_tab);
/* The gfx950 code object of the stepper module (cf. llvm_state::get_object_code(), include/heyoka/llvm_state.hpp) and a
 * plain hiprtc compilation of a HIP source with the options of the steppers (for offline inspection: disassembly, the
 * code-generation checks of tests/test_codegen_hazards.py). Two-call convention: out == NULL -> *size receives the size. */
int hy_tab_get_code_object(hy_tab, void *out, size_t *size);
int hy_hiprtc_compile(const char *source, void *out, size_t *size);

int hy_tab_get_state(hy_tab, double *out);                 /* get_state()        n_eq * batch_size */
int hy_tab_set_state(hy_tab, const double *in);            /* the values of get_state_data()[...] = in[...]; by value: the
                                                            * integrator stays lazily synchronised */
int hy_tab_get_pars(hy_tab, double *out);                  /* get_pars() */
int hy_tab_set_pars(hy_tab, const double *in);             /* like hy_tab_set_state() for get_pars_data() */
/* get_state_data() / get_pars_data() (include/heyoka/taylor.hpp:984-990): MUTABLE pointers to the host mirrors, valid for
 * the lifetime of the integrator. Reference call sites write through them between steps (ta.get_state_data()[i] = ...), so
 * handing one out switches the integrator to eager synchronisation: the mirrors are refreshed after every launch and
 * uploaded before the next one (a download of the whole state per step: use the setters above, or the device views of
 * hy_tab_device_ptr(), where that matters). NULL + hy_last_error() on failure. */
double *hy_tab_get_state_data(hy_tab);
double *hy_tab_get_pars_data(hy_tab);
int hy_tab_get_dtime(hy_tab, double *hi, double *lo);      /* get_dtime()        batch_size each; lo may be NULL */
int hy_tab_set_time(hy_tab, const double *t, size_t n);    /* set_time(): n == 1 scalar, else batch_size */
int hy_tab_set_dtime(hy_tab, const double *hi, const double *lo, size_t n); /* set_dtime() */
int hy_tab_get_tc(hy_tab, double *out);                    /* get_tc()           n_eq * (order + 1) * batch_size: the
                                                            * coefficients of the last step taken with write_tc (zeros
                                                            * before the first one), like the reference's m_tc */
int hy_tab_get_last_h(hy_tab, double *out);                /* get_last_h() */
/* update_d_output(t, rel_time) (src/taylor_adaptive_batch.cpp:2251-2327): n == 1 scalar, else batch_size. */
int hy_tab_update_d_output(hy_tab, const double *t, size_t n, int rel_time, double *out);

/* step() / step_backward() / step(max_delta_ts) (taylor.hpp:1001-1003; step_impl()
 * src/taylor_adaptive_batch.cpp:632-727). */
int hy_tab_step(hy_tab, int write_tc);
int hy_tab_step_backward(hy_tab, int write_tc);
int hy_tab_step_limited(hy_tab, const double *max_delta_ts, size_t n, int write_tc);
int hy_tab_get_step_res(hy_tab, int64_t *outcome, double *h); /* get_step_res() */

/* Step callback: bool(taylor_adaptive_batch &) (include/heyoka/step_callback.hpp:59-62).
 * Return non-zero to continue, 0 to stop (outcome cb_stop). */
typedef int (*hy_step_callback)(hy_tab, void *user_data);

/* propagate_until() / propagate_for() (taylor.hpp:1064-1107; propagate_until_impl()
 * src/taylor_adaptive_batch.cpp:1137-1534, propagate_for_impl() :1082-1118).
 *  ts / n_ts ............ final times (durations for propagate_for): n_ts == 1 scalar, else batch_size
 *  max_steps ............ kw::max_steps (0 = unlimited)
 *  max_delta_ts / n_mdt . kw::max_delta_t: n_mdt == 0 none, 1 scalar, else batch_size
 *  cb ................... kw::callback (NULL = none). Without a callback the whole propagation runs
 *                         device-resident in one kernel launch; with a callback the reference's
 *                         lock-step loop is used (one launch per step, callback on the host).
 *  write_tc, c_output ... kw::write_tc, kw::c_output. With c_output != 0 the lock-step loop is used as well and
 *                         the continuous output object is retrieved with hy_tab_take_c_output(). */
int hy_tab_propagate_until(hy_tab, const double *ts, size_t n_ts, uint64_t max_steps, const double *max_delta_ts,
                           size_t n_mdt, hy_step_callback cb, void *cb_data, int write_tc, int c_output);
int hy_tab_propagate_for(hy_tab, const double *dts, size_t n_dts, uint64_t max_steps, const double *max_delta_ts,
                         size_t n_mdt, hy_step_callback cb, void *cb_data, int write_tc, int c_output);
/* The full step-callback protocol (include/heyoka/step_callback.hpp:46-62, :139-185): a callback may provide a
 * pre_hook(), run once after the validation of the arguments and before the first step
 * (src/taylor_adaptive_batch.cpp:1356-1365, :1782-1791; it must not move the time coordinate), and kw::callback accepts a
 * range of callbacks, which form a set: every member runs at every step and the results are and-ed
 * (src/step_callback.cpp:108-127); a NULL `call` inside a set of more than one member is an error
 * ("Cannot construct a callback set containing one or more empty callbacks"), n_cbs == 0 means no callback. */
/* A pre-hook returns 0, or non-zero to abort the propagation before its first step (how an exception thrown by
 * pre_hook() travels through the C boundary; the reference lets it propagate out of propagate_*()); a `call` member
 * may return a NEGATIVE value for the same purpose: the remaining members of the set are not run and the propagation
 * stops like after a `false`. */
typedef int (*hy_step_pre_hook)(hy_tab, void *user_data);
typedef struct {
    hy_step_callback call;
    hy_step_pre_hook pre_hook; /* NULL: the default no-op */
    void *user_data;
} hy_step_callback_desc;
int hy_tab_propagate_until_cbs(hy_tab, const double *ts, size_t n_ts, uint64_t max_steps, const double *max_delta_ts,
                               size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, int write_tc, int c_output);
int hy_tab_propagate_for_cbs(hy_tab, const double *dts, size_t n_dts, uint64_t max_steps, const double *max_delta_ts,
                             size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, int write_tc, int c_output);
int hy_tab_propagate_grid_cbs(hy_tab, const double *grid, size_t n_grid, uint64_t max_steps, const double *max_delta_ts,
                              size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, double *out);
/* callback::angle_reducer (include/heyoka/callback/angle_reducer.hpp, src/callback/angle_reducer.cpp): the step callback which
 * keeps the named state variables in [0, 2 pi), x -= twopi * floor(x / twopi) with twopi = 0x1.921fb54442d18p+2 and every
 * operation rounded (no FMA); non-finite values are left alone. hy_angle_reducer_new() fails (NULL, hy_last_error()) on an
 * empty list or a non-variable; hy_angle_reducer_new_default() gives the default-constructed object, which every use rejects.
 * hy_angle_reducer_call / hy_angle_reducer_pre_hook are ready-made members for a hy_step_callback_desc with the handle as
 * user_data. The library recognises them by address: the reduction runs on the device over the device-resident state
 * (kernel hy_angle_reduce after every sweep), and when every member of the callback set is one, propagate_until() /
 * propagate_for() without continuous output on an integrator without events run ONE launch of a stepper variant which
 * reduces inside the propagate kernel (generators: straight-line, table, first-generation / multi-class wave-cluster). */
typedef struct hy_angle_reducer_s *hy_angle_reducer;
hy_angle_reducer hy_angle_reducer_new(const hy_expr *vars, size_t n);
hy_angle_reducer hy_angle_reducer_new_default(void);
hy_angle_reducer hy_angle_reducer_clone(hy_angle_reducer);
void hy_angle_reducer_free(hy_angle_reducer);
/* "Angle reducer: {x, y}" / "Angle reducer (default constructed)". Caller frees. */
char *hy_angle_reducer_str(hy_angle_reducer);
int hy_angle_reducer_call(hy_tab, void *user);     /* 1, or -1 on error (hy_last_error()) */
int hy_angle_reducer_pre_hook(hy_tab, void *user); /* 0, or 1 on error */
/* How the step callback of the last propagate_*() ran: 0 none, 1 host callback after every sweep, 2 angle reduction on the
 * device after every sweep, 3 angle reduction fused into the propagate kernel, 4 every member of the callback set is
 * library-side - step actions and angle reducers, at least one action - and was applied on the device after every sweep. */
int hy_tab_last_callback_path(hy_tab);
/* step_action (MI355X extension, no counterpart in the reference; heyoka_amd/csrc/step_action.hpp): a step callback defined by
 * assignments `state variable <- expression` and an optional stop condition, applied by a generated kernel (hy_step_action,
 * one lane per system) over the device-resident state after every sweep - the sibling of hy_event_action in the
 * step-callback slot. The expressions may read state variables, par[...], the time (time_hi after the step) and numbers; all
 * of them, the condition included, read the state from BEFORE the action. It acts on the systems whose last step had
 * non-zero length; the values are bit for bit those of a hy_cfunc of the same expressions over the state variables; Taylor
 * coefficients, last_h, times, cooldowns and the event log are left alone. stop_when (may be NULL; n may be 0 if it is not)
 * holds for a system when its value c satisfies !(c == 0): with batch_semantics 0, 1, 2 the callback returns 0 and the loop
 * ends as after a host callback which returned false; with batch_semantics 3 the system is retired alone with the sticky
 * outcome cb_stop and the others carry on (hy_tab_get_n_stopped_by_action(): their number in the last call; they are not
 * counted by hy_tab_get_n_retired()). hy_step_action_new() fails (NULL, hy_last_error()) on a left-hand side which is not a
 * variable and without assignments and condition; the checks against the system of an integrator - a left-hand side which
 * is not a state variable or is repeated, a variable which is not a state variable, a par[i] the integrator does not have -
 * are made when the action first meets it (HY_ERR_INVALID_ARGUMENT from the propagate call, -1 from a direct call).
 * hy_step_action_call is the ready-made member for a hy_step_callback_desc with the handle as user_data (no pre-hook),
 * recognised by address: 1 to continue, 0 to stop, -1 on error (hy_last_error()). */
typedef struct hy_step_action_s *hy_step_action;
hy_step_action hy_step_action_new(const hy_expr *vars, const hy_expr *rhs, size_t n, hy_expr stop_when);
hy_step_action hy_step_action_clone(hy_step_action);
void hy_step_action_free(hy_step_action);
/* "step_action({v: (0.999 * v)}, stop_when=...)". Caller frees. */
char *hy_step_action_str(hy_step_action);
int hy_step_action_call(hy_tab, void *user);
uint64_t hy_tab_get_n_stopped_by_action(hy_tab);
/* With hy_tab_set_event_timing(on): sum of the durations (ms, HIP events) of the hy_step_action launches and their number. */
int hy_tab_step_action_kernel_ms(hy_tab, double *ms, uint64_t *launches);
/* INTERNAL hooks of the test suite: the HIP source of the module of an action for a system (no integrator, no GPU; caller
 * frees), and source (caller frees) / gfx950 code object (owned by the library) of the module inside an integrator. */
char *hy_step_action_source(hy_sys, hy_step_action);
int hy_tab_step_action_module(hy_tab, hy_step_action, char **source, const char **data, size_t *size);
/* Beyond the constructor, the destructor and the two ready-made members: hy_angle_reducer_new_default / _clone / _str serve
 * the language bindings (default construction, copy, repr). The four entry points below are INTERNAL hooks of the test suite and
 * of the build-time compilation check, not part of the supported interface. */
/* Source of the stepper variant with the reduction of the state variables idx[0..n) (sorted) fused in; "" and the reason in
 * *why_not (may be NULL) when the generator of this integrator declines. Seconds of its last compilation. Caller frees. */
char *hy_tab_angle_reduce_variant_source(hy_tab, const uint32_t *idx, size_t n, char **why_not);
double hy_tab_angle_reduce_compile_seconds(hy_tab);
/* Source of the module of the stand-alone kernel hy_angle_reduce, and the same arithmetic on the host. Caller frees. */
char *hy_angle_reduce_source(void);
double hy_angle_reduce_host(double x);
/* ------------------------------------------------------------------------------------------------
 * continuous_output_batch<double> (include/heyoka/continuous_output.hpp:151-204,
 * src/continuous_output.cpp:602-1236): the optional<continuous_output_batch> slot of the tuple returned
 * by propagate_for/until(). Coefficients and times stay in HBM; evaluation is one kernel launch. */
typedef struct hy_cout_s *hy_cout;
/* Moves the continuous output recorded by the last propagate_for/until(c_output != 0) into *out
 * (*out = NULL if no step was taken, like the empty optional of the reference). Free with hy_cout_free(). */
int hy_tab_take_c_output(hy_tab, hy_cout *out);
void hy_cout_free(hy_cout);
/* Copy (the device data is shared, the output buffers are not). */
hy_cout hy_cout_clone(hy_cout);
/* operator()(T) (n_tm == 1), operator()(const std::vector<T> &) (n_tm == batch_size; any other size is
 * an error). out receives get_output(): n_eq * batch_size values, out[var * batch_size + lane]. */
int hy_cout_eval(hy_cout, const double *tm, size_t n_tm, double *out);
/* MI355X extension: target times d_tm[batch_size] and d_out[n_eq * batch_size] in device memory;
 * asynchronous on the integrator's stream. */
int hy_cout_eval_device(hy_cout, const double *d_tm, double *d_out);
uint32_t hy_cout_get_batch_size(hy_cout);
uint32_t hy_cout_get_dim(hy_cout);
uint32_t hy_cout_get_order(hy_cout);
/* get_n_steps() (padding excluded). */
int hy_cout_get_n_steps(hy_cout, size_t *n_steps);
/* get_bounds(): lb[batch_size], ub[batch_size]. */
int hy_cout_get_bounds(hy_cout, double *lb, double *ub);
/* get_times(): (n_steps + 2) * batch_size values (last row = +-inf padding); lo may be NULL. */
int hy_cout_get_times(hy_cout, double *hi, double *lo);
/* get_tcs(): n_steps * n_eq * (order + 1) * batch_size values, downloaded from the device. */
int hy_cout_get_tcs(hy_cout, double *out);
/* operator<<: malloc'ed string, free with hy_free_str(). */
char *hy_cout_to_string(hy_cout);

/* propagate_grid() (taylor.hpp:1113-1119; propagate_grid_impl() src/taylor_adaptive_batch.cpp:1546-2055).
 * grid: n_grid * batch_size values laid out grid[point * batch_size + lane];
 * out: n_grid * n_eq * batch_size values (NaN where not reached). */
int hy_tab_propagate_grid(hy_tab, const double *grid, size_t n_grid, uint64_t max_steps, const double *max_delta_ts,
                          size_t n_mdt, hy_step_callback cb, void *cb_data, double *out);
/* MI355X extension of propagate_grid() for ensemble-scale batches: the n_grid * n_eq * batch_size samples are
 * written to a caller-owned device buffer d_out (same layout as above) instead of a host vector; no callback.
 * scalar_grid != 0: grid holds n_grid values used by every lane (the splat of ensemble_propagate_grid_batch(),
 * src/ensemble_propagate.cpp:266-273), otherwise n_grid * batch_size values. */
int hy_tab_propagate_grid_device(hy_tab, const double *grid, size_t n_grid, int scalar_grid, uint64_t max_steps,
                                 const double *max_delta_ts, size_t n_mdt, double *d_out);
/* Grid observables (MI355X extension, no counterpart in the reference; heyoka_amd/csrc/grid_observables.hpp): n_obs expressions
 * over the state variables of the system, par[...] and the time. out holds n_grid * n_obs * batch_size values laid out
 * out[(point * n_obs + observable) * batch_size + lane] - the layout of hy_tab_propagate_grid() with n_eq replaced by n_obs.
 * The post-step kernel of the grid loop evaluates the dense output of the state rows the observables read and the
 * observables themselves: a reached row holds, bit for bit, what a hy_cfunc of the same expressions over the state variables
 * returns for the state sample hy_tab_propagate_grid() writes for that row, the parameters of the lane and the grid time of
 * the row and lane; a row which was not reached (step limit, callback stop, non-finite lane, retired system) is NaN in every
 * column. State, times, outcomes, step counts, min / max |h| and Taylor coefficients are those of the call without
 * observables. cbs / n_cbs as in hy_tab_propagate_grid_cbs() (NULL / 0: no callback). HY_ERR_INVALID_ARGUMENT before
 * anything runs for a null handle, a null expression, an empty list, a variable which is not a state variable and a par[i]
 * the integrator does not have. */
int hy_tab_propagate_grid_obs(hy_tab, const double *grid, size_t n_grid, uint64_t max_steps, const double *max_delta_ts,
                              size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, const hy_expr *obs, size_t n_obs,
                              double *out);
/* The same into a caller-owned device buffer d_out of n_grid * n_obs * batch_size doubles; no callback; scalar_grid as in
 * hy_tab_propagate_grid_device(). */
int hy_tab_propagate_grid_obs_device(hy_tab, const double *grid, size_t n_grid, int scalar_grid, uint64_t max_steps,
                                     const double *max_delta_ts, size_t n_mdt, const hy_expr *obs, size_t n_obs, double *d_out);
/* INTERNAL hooks of the test suite: the HIP source of the post-step module with the section of the observables (kernels
 * hy_grid_post, hy_grid_obs0, hy_grid_unsample) for a system, without an integrator and without a GPU (caller frees; NULL
 * and hy_last_error() on error), and source (caller frees) / gfx950 code object (owned by the library) of the module
 * inside an integrator. HEYOKA_AMD_GRID_OBS=registers|staged overrides how the kernel holds the samples of a grid point. */
char *hy_grid_obs_source(hy_sys, const hy_expr *obs, size_t n_obs, uint32_t order, int high_accuracy);
int hy_tab_grid_obs_module(hy_tab, const hy_expr *obs, size_t n_obs, char **source, const char **data, size_t *size);
/* Grid statistics (MI355X extension): the observables are not stored per grid point but folded, per observable and system, over
 * the grid points the system reaches - the rows of hy_tab_propagate_grid_obs() which are not NaN fill, a prefix of its grid -
 * in ascending order. With y the value at a point and t the grid time of the row and lane:
 *   MIN / MAX      start with the first value; then the value replaces the extremum m if y < m (y > m) or m != m: NaN values are
 *                  ignored unless all are NaN, -0.0 does not replace +0.0;
 *   T_MIN / T_MAX  the first grid time at which the current minimum / maximum was attained;
 *   SUM            one rounded addition per point, in this order (NaN propagates);
 *   LAST           the value at the last point reached;   COUNT   the number of points reached, as a double.
 * A system which reached no point (the call returned before its first grid point) has NaN everywhere and COUNT 0. out holds
 * n_obs * n_stats * batch_size values, out[(observable * n_stats + statistic) * batch_size + lane], statistics in the order of
 * stats; nothing of the size of the grid is allocated for the output on the host or on the device. The integrator is left,
 * bit for bit, as by hy_tab_propagate_grid_obs(). HY_ERR_INVALID_ARGUMENT before anything runs: as for the _obs functions,
 * and for a null or empty list of statistics, an unknown code and a statistic named twice. */
#define HY_GRID_STAT_MIN 0
#define HY_GRID_STAT_MAX 1
#define HY_GRID_STAT_T_MIN 2
#define HY_GRID_STAT_T_MAX 3
#define HY_GRID_STAT_SUM 4
#define HY_GRID_STAT_LAST 5
#define HY_GRID_STAT_COUNT 6
int hy_tab_propagate_grid_stats(hy_tab, const double *grid, size_t n_grid, uint64_t max_steps, const double *max_delta_ts,
                                size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, const hy_expr *obs, size_t n_obs,
                                const int *stats, size_t n_stats, double *out);
/* The same into a caller-owned device buffer d_out of n_obs * n_stats * batch_size doubles; no callback. */
int hy_tab_propagate_grid_stats_device(hy_tab, const double *grid, size_t n_grid, int scalar_grid, uint64_t max_steps,
                                       const double *max_delta_ts, size_t n_mdt, const hy_expr *obs, size_t n_obs,
                                       const int *stats, size_t n_stats, double *d_out);
/* INTERNAL hooks of the test suite, the counterparts of hy_grid_obs_source() / hy_tab_grid_obs_module() for the module which
 * folds (hy_grid_post merges, hy_grid_obs0 starts the accumulators, hy_grid_unsample restores them). */
char *hy_grid_stats_source(hy_sys, const hy_expr *obs, size_t n_obs, const int *stats, size_t n_stats, uint32_t order,
                           int high_accuracy);
int hy_tab_grid_stats_module(hy_tab, const hy_expr *obs, size_t n_obs, const int *stats, size_t n_stats, char **source,
                             const char **data, size_t *size);
/* Ensemble statistics (MI355X extension): the observables are folded ACROSS the systems, per grid point and observable. With
 * Y[g][o][i] the output of hy_tab_propagate_grid_obs() and V the entries of Y[g][o][:] which are not NaN (fill or computed):
 *   COUNT      the size of V, as a double;
 *   MIN / MAX  the extremum of V in the total order -inf < ... < -0.0 < +0.0 < ... < +inf; NaN if V is empty;
 *   SUM        the EXACT sum of V, rounded once to nearest-even: +0.0 for an exact zero or an empty V, +-inf beyond the largest
 *              double, +inf (-inf) if V holds +inf (-inf), NaN if it holds both;
 *   SUM_SQ     the same over y * y, one rounded multiplication per value (a product which overflows counts as +inf);
 *   MEAN       SUM / COUNT, one division; NaN if COUNT is 0.
 * The variance is the caller's: (SUM_SQ - SUM * SUM / COUNT) / COUNT cancels when the spread is small next to the mean.
 * The accumulators are integers updated with integer atomics, so the values do not depend on the order of the systems, on the
 * launches, on the sharding of an ensemble: hy_tab_propagate_grid_ens() writes the words of the accumulators - acc holds
 * hy_grid_ens_acc_words() words, a record per (g, o) in this order whose size depends on the list alone -, the accumulators
 * of the shards of an ensemble are added with hy_grid_ens_merge() (at most 2^30 values per record over everything merged),
 * and hy_grid_ens_finish() rounds them: out[(g * n_obs + o) * n_stats + k], statistics in the order of stats. The integrator
 * is left, bit for bit, as by hy_tab_propagate_grid_obs(). HY_ERR_INVALID_ARGUMENT before anything runs: as for the _obs
 * functions, and for a null or empty list of statistics, an unknown code and a statistic named twice.
 * HEYOKA_AMD_GRID_ENS=peratomic: one atomic per lane and word instead of one per wavefront and word; the same words. */
#define HY_ENS_STAT_COUNT 0
#define HY_ENS_STAT_MIN 1
#define HY_ENS_STAT_MAX 2
#define HY_ENS_STAT_SUM 3
#define HY_ENS_STAT_SUM_SQ 4
#define HY_ENS_STAT_MEAN 5
int hy_tab_propagate_grid_ens(hy_tab, const double *grid, size_t n_grid, uint64_t max_steps, const double *max_delta_ts,
                              size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, const hy_expr *obs, size_t n_obs,
                              const int *stats, size_t n_stats, uint64_t *acc);
/* The same into a caller-owned device buffer d_acc of hy_grid_ens_acc_words() words; no callback. */
int hy_tab_propagate_grid_ens_device(hy_tab, const double *grid, size_t n_grid, int scalar_grid, uint64_t max_steps,
                                     const double *max_delta_ts, size_t n_mdt, const hy_expr *obs, size_t n_obs,
                                     const int *stats, size_t n_stats, uint64_t *d_acc);
/* The number of 64-bit words of the accumulators of n_grid points and n_obs observables (0 and hy_last_error() on error). */
size_t hy_grid_ens_acc_words(size_t n_grid, size_t n_obs, const int *stats, size_t n_stats);
/* On the host: accumulators in their start state; one value y into the record (g, o) - the twin of what the kernel does per
 * system, for those who fold by hand -; dst += src; the values of the accumulators. */
int hy_grid_ens_init(uint64_t *acc, size_t n_grid, size_t n_obs, const int *stats, size_t n_stats);
int hy_grid_ens_add(uint64_t *acc, size_t n_grid, size_t n_obs, const int *stats, size_t n_stats, size_t g, size_t o, double y);
int hy_grid_ens_merge(uint64_t *dst, const uint64_t *src, size_t n_grid, size_t n_obs, const int *stats, size_t n_stats);
int hy_grid_ens_finish(const uint64_t *acc, size_t n_grid, size_t n_obs, const int *stats, size_t n_stats, double *out);
/* INTERNAL hooks of the test suite, the counterparts of hy_grid_stats_source() / hy_tab_grid_stats_module() for the module
 * which merges across the systems (hy_grid_post and hy_grid_obs0 merge; there is no hy_grid_unsample). */
char *hy_grid_ens_source(hy_sys, const hy_expr *obs, size_t n_obs, const int *stats, size_t n_stats, uint32_t order,
                         int high_accuracy);
int hy_tab_grid_ens_module(hy_tab, const hy_expr *obs, size_t n_obs, const int *stats, size_t n_stats, char **source,
                           const char **data, size_t *size);
/* Ensemble histograms (MI355X extension): the observables are binned ACROSS the systems, per grid point. n_edges[o] is the
 * number of bin edges of observable o - 0: no histogram for it -, and edges holds the lists one behind the other: E[0] < ... <
 * E[B], finite, B = n_edges[o] - 1 bins, 1 <= B <= 4096. With Y[g][o][i] the output of hy_tab_propagate_grid_obs(), every
 * Y[g][o][i] which is not NaN is counted in the slot s = #{ j : E[j] <= y } of the record of (g, o), by comparisons alone -
 * numpy.searchsorted(E, y, side="right"): slot 0 is the underflow (-inf included), slots 1 ... B are the bins [E[s-1], E[s]),
 * slot B + 1 is the overflow (y >= E[B], +inf included); -0.0 and +0.0 share a slot. A record is B + 2 unsigned 64-bit
 * counters in slot order; the records of a grid point follow each other in the order of the observables with edges, and
 * acc_hist holds hy_grid_hist_acc_words() words, grid point after grid point. The counters do not depend on the order of the
 * systems, on the launches, on the sharding of an ensemble: those of shards are added with hy_grid_hist_merge().
 * n_stats != 0: the ensemble statistics of hy_tab_propagate_grid_ens() in the same call, and acc_ens receives the words that
 * call writes; n_stats == 0: none, and acc_ens is null. The integrator is left, bit for bit, as by
 * hy_tab_propagate_grid_obs(). HY_ERR_INVALID_ARGUMENT before anything runs: as for the _ens functions, and for no edges at all,
 * a list of one edge, edges which are not finite and strictly increasing, more than 4096 bins.
 * HEYOKA_AMD_GRID_HIST=peratomic|aggregate|hybrid: how the lanes of a wavefront merge their counts (one atomic per lane; one per
 * group of lanes with the same word; K turns of the latter, then the former - the default); the same words.
 * HEYOKA_AMD_GRID_HIST_TURNS=1|2|4 overrides the K the library was built with: the switch of the measurement behind that choice,
 * any other value is refused. */
int hy_tab_propagate_grid_hist(hy_tab, const double *grid, size_t n_grid, uint64_t max_steps, const double *max_delta_ts,
                               size_t n_mdt, const hy_step_callback_desc *cbs, size_t n_cbs, const hy_expr *obs, size_t n_obs,
                               const int *stats, size_t n_stats, const double *edges, const size_t *n_edges, uint64_t *acc_ens,
                               uint64_t *acc_hist);
/* The same into a caller-owned device buffer d_acc: the hy_grid_ens_acc_words() words of the ensemble statistics (none if
 * n_stats is 0) followed by the hy_grid_hist_acc_words() words of the histograms; no callback. */
int hy_tab_propagate_grid_hist_device(hy_tab, const double *grid, size_t n_grid, int scalar_grid, uint64_t max_steps,
                                      const double *max_delta_ts, size_t n_mdt, const hy_expr *obs, size_t n_obs,
                                      const int *stats, size_t n_stats, const double *edges, const size_t *n_edges,
                                      uint64_t *d_acc);
/* The number of 64-bit words of the histograms of n_grid points (0 and hy_last_error() on error). */
size_t hy_grid_hist_acc_words(size_t n_grid, size_t n_obs, const size_t *n_edges);
/* On the host: counters in their start state; one value y into the record (g, o) - the twin of what the kernel does per
 * system -; dst += src; per grid point g the smallest slot of observable o whose cumulative count reaches the 1-based rank
 * k[g] (slot[g] = -1 if k[g] is 0 or larger than the number of values counted). hy_grid_hist_add() checks the numbers of
 * edges, not their values: give it edges which a call of hy_tab_propagate_grid_hist() would accept. */
int hy_grid_hist_init(uint64_t *acc, size_t n_grid, size_t n_obs, const size_t *n_edges);
int hy_grid_hist_add(uint64_t *acc, size_t n_grid, size_t n_obs, const double *edges, const size_t *n_edges, size_t g, size_t o,
                     double y);
int hy_grid_hist_merge(uint64_t *dst, const uint64_t *src, size_t n_grid, size_t n_obs, const size_t *n_edges);
int hy_grid_hist_rank_slot(const uint64_t *acc, size_t n_grid, size_t n_obs, const size_t *n_edges, size_t o, const uint64_t *k,
                           int64_t *slot);
/* INTERNAL hooks of the test suite, the counterparts of hy_grid_ens_source() / hy_tab_grid_ens_module() for the module which
 * counts into histograms, with or without ensemble statistics (n_stats == 0). The text depends on the numbers of edges, not on
 * their values. */
char *hy_grid_hist_source(hy_sys, const hy_expr *obs, size_t n_obs, const int *stats, size_t n_stats, const double *edges,
                          const size_t *n_edges, uint32_t order, int high_accuracy);
int hy_tab_grid_hist_module(hy_tab, const hy_expr *obs, size_t n_obs, const int *stats, size_t n_stats, const double *edges,
                            const size_t *n_edges, char **source, const char **data, size_t *size);
/* get_propagate_res(): (outcome, min |h|, max |h|, n_steps) per lane. */
int hy_tab_get_propagate_res(hy_tab, int64_t *outcome, double *min_h, double *max_h, uint64_t *n_steps);

/* ------------------------------------------------------------------------------------------------
 * Device-resident access (MI355X extension; the reference has no device boundary).
 * --------------------------------------------------------------------------------------------- */
#define HY_BUF_STATE 0   /* double[n_eq * batch_size] */
#define HY_BUF_PARS 1    /* double[n_pars * batch_size] */
#define HY_BUF_TIME_HI 2 /* double[batch_size] */
#define HY_BUF_TIME_LO 3 /* double[batch_size] */
#define HY_BUF_TC 4      /* double[n_eq * (order + 1) * batch_size] */
#define HY_BUF_N_STEPS 5 /* uint64[batch_size]: step counters of the last propagate_*() */
#define HY_BUF_OUTCOME 6 /* int64[batch_size]: taylor_outcome of the last step()/propagate_*() */
#define HY_BUF_LAST_H 7  /* double[batch_size] */
/* Device pointer of one of the SoA arrays of the integrator (uploads pending host changes first). */
void *hy_tab_device_ptr(hy_tab, int which);
/* Tell the integrator that the caller wrote to the device arrays. */
int hy_tab_mark_device_modified(hy_tab);
/* Run all subsequent kernels/copies on the given hipStream_t (NULL = default stream). */
int hy_tab_set_stream(hy_tab, void *hip_stream);
int hy_tab_synchronize(hy_tab);
/* Sum over lanes of the step counters of the last propagate_*() call. */
uint64_t hy_tab_get_last_total_steps(hy_tab);
/* Durations (ms) of the last (at most) n stepper-kernel launches, oldest first, measured with HIP
 * events recorded on the launch stream immediately around each launch. Returns the count written. */
size_t hy_tab_get_kernel_ms_history(hy_tab, double *out, size_t n);

/* Stepper function-pointer ABI of the reference
 * (`void step(T *state, const T *pars, const T *time, T *h, T *tc)`,
 *  include/heyoka/detail/ta_jit_data.hpp:35-44, looked up at src/taylor_adaptive_batch.cpp:2391-2393)
 * on caller-owned device buffers holding n_systems systems:
 *   d_state rw [n_eq * n], d_pars [n_pars * n] (may be NULL if no parameters), d_time [n] (hi part),
 *   d_h in: signed max step (+-inf allowed), out: step taken [n], d_tc nullable [n_eq * (order+1) * n].
 * No error channel for numerical failures (non-finite results are the caller's to detect). */
int hy_tab_raw_step(hy_tab, double *d_state, const double *d_pars, const double *d_time, double *d_h, double *d_tc,
                    uint64_t n_systems);
/* The other pointer types of the reference's stepper ABI (include/heyoka/detail/ta_jit_data.hpp:34-43), same argument
 * order, on caller-owned device buffers of n_systems systems:
 *   step_f_e_t   (jet, state, pars, time, h, max_abs_state): the stepper with events of an integrator constructed with
 *                events (taylor_add_adaptive_step_with_events(), src/taylor_00.cpp:592-710) - d_jet receives the Taylor
 *                coefficients of the state variables, [n_eq * (order + 1) * n], followed by those of the event equations,
 *                [(n_t_events + n_nt_events) * (order + 1) * n] (terminal events first), d_h in: signed max step, out: the
 *                step size of the selector, d_max_abs_state [n]: max |x_i| over the state; the state is NOT updated;
 *   d_out_f_t    (d_out, tc, h): dense output (taylor_add_d_out_function(), src/taylor_01.cpp:1015-1185) - d_out [n_eq * n]
 *                = the Taylor polynomials d_tc [n_eq * (order + 1) * n] evaluated at d_h [n] (compensated in high-accuracy
 *                mode, Horner otherwise);
 *   c_step_f_t / c_step_f_e_t (... , void *tape): the same two steppers with the tape in caller-owned device memory of
 *                hy_tab_tape_size_align() bytes (0: this stepper keeps its coefficients on chip and ignores the argument;
 *                src/taylor_02.cpp:1194-1260 for the reference's tape). */
int hy_tab_raw_step_e(hy_tab, double *d_jet, const double *d_state, const double *d_pars, const double *d_time, double *d_h,
                      double *d_max_abs_state, uint64_t n_systems);
int hy_tab_raw_d_out_f(hy_tab, double *d_out, const double *d_tc, const double *d_h, uint64_t n_systems);
int hy_tab_raw_step_tape(hy_tab, double *d_state, const double *d_pars, const double *d_time, double *d_h, double *d_tc,
                         void *d_tape, uint64_t n_systems);
int hy_tab_raw_step_e_tape(hy_tab, double *d_jet, const double *d_state, const double *d_pars, const double *d_time,
                           double *d_h, double *d_max_abs_state, void *d_tape, uint64_t n_systems);
int hy_tab_tape_size_align(hy_tab, uint64_t n_systems, size_t *size, size_t *align);

/* Build-time check: hiprtc-compiles for gfx950 the auxiliary kernels that are otherwise compiled at first use on a
 * GPU (continuous output, propagate_grid post-step, event detection) for the given order / dimension; does not need
 * a GPU. Returns HY_OK or an error code (hy_last_error()). */
int hy_compile_aux_kernels(uint32_t order, uint32_t dim, int high_accuracy);

/* ------------------------------------------------------------------------------------------------
 * cfunc<double> (include/heyoka/expression.hpp:735-970, src/cfunc_class.cpp, function_decompose()
 * src/expression_cfunc.cpp:723-900): compiled evaluation of fn(vars) over many input columns.
 * One HIP kernel, one lane per evaluation, on SoA arrays in[var * nevals + eval] (the row-major 2D
 * layout of the reference's multi-evaluation call operator, which is also the integrator's state
 * layout: the device-side invariant monitor of an ensemble is hy_cfunc_eval_device() on
 * hy_tab_device_ptr(HY_BUF_STATE)). */
typedef struct hy_cfunc_s *hy_cfunc;
hy_cfunc hy_cfunc_new(const hy_expr *fn, size_t n_fn, const hy_expr *vars, size_t n_vars, int device);
void hy_cfunc_free(hy_cfunc);
uint32_t hy_cfunc_get_nparams(hy_cfunc);
uint32_t hy_cfunc_get_nvars(hy_cfunc);
uint32_t hy_cfunc_get_nouts(hy_cfunc);
int hy_cfunc_is_time_dependent(hy_cfunc);
/* get_dc() in textual form / generated HIP source; caller frees with hy_free_str(). */
char *hy_cfunc_decomposition_str(hy_cfunc);
char *hy_cfunc_get_hip_source(hy_cfunc);
int hy_cfunc_set_stream(hy_cfunc, void *hip_stream);
/* Call operator on host arrays: out_size = nouts * nevals, in_size = nvars * nevals, pars
 * (nparams * nevals; NULL if none), time (nevals; NULL if none). */
int hy_cfunc_eval(hy_cfunc, double *out, size_t out_size, const double *in, size_t in_size, const double *pars,
                  size_t pars_size, const double *time, size_t time_size);
/* Same on device-resident arrays, asynchronous on the stream. */
int hy_cfunc_eval_device(hy_cfunc, double *d_out, const double *d_in, const double *d_pars, const double *d_time,
                         uint64_t nevals);

/* ------------------------------------------------------------------------------------------------
 * ensemble_propagate_until_batch() (include/heyoka/ensemble_propagate.hpp:222-237,
 * src/ensemble_propagate.cpp:193-222): n_iter independent propagations of copies of `ta`.
 *  gen(ta_copy, iteration, user_data): sets the initial conditions of the copy (on the host),
 *      returns 0 on success. Invoked serially on the calling thread.
 *  Iterations are distributed round-robin over `n_devices` HIP devices (0 = all visible), one host
 *  thread per device; n_devices = -k: k host threads spread round-robin over the visible devices (more
 *  workers than devices). The propagated copies are returned in out[0..n_iter) (caller frees each with
 *  hy_tab_free()); every copy lives on the device which propagated it and its getters fetch from there. */
typedef int (*hy_ensemble_gen)(hy_tab ta_copy, size_t iteration, void *user_data);
int hy_ensemble_propagate_until_batch(hy_tab ta, double t, size_t n_iter, hy_ensemble_gen gen, void *gen_data,
                                      uint64_t max_steps, int n_devices, hy_tab *out);
int hy_ensemble_propagate_for_batch(hy_tab ta, double delta_t, size_t n_iter, hy_ensemble_gen gen, void *gen_data,
                                    uint64_t max_steps, int n_devices, hy_tab *out);
/* The final states of n integrators (e.g. the copies returned above, each on the device which propagated it) gathered
 * into ONE buffer: out[row * n_total + offset_i + lane], n_total = sum of the batch sizes, offset_i = sum of those of the
 * integrators before i; out is host memory (out_is_device = 0) or memory of device dst_device. Between devices the
 * blocks travel through RCCL (librccl loaded at run time: ncclSend / ncclRecv over xGMI inside one group; set
 * HEYOKA_AMD_GATHER_RCCL=1 to take that route on a single device too, =0 to force plain device-to-device copies, which are
 * also the fallback when librccl is absent). *used_rccl (may be NULL) reports the route taken. The reference returns the
 * iterations in host memory of one process (src/ensemble_propagate.cpp:193-297): this is how a caller of the drop-in gets
 * the 8-GPU ensemble in one place. */
int hy_ensemble_gather_states(const hy_tab *tabs, size_t n, int dst_device, double *out, size_t out_doubles,
                              int out_is_device, int *used_rccl);
/* The same gather with everything the reference's returned integrators hold (src/ensemble_propagate.cpp:193-297: m_state,
 * m_time_hi / m_time_lo, m_prop_res): out receives (dim + 6) rows of n_total 8-byte words, out[row * n_total + offset_i +
 * lane] - the dim state rows, then time_hi, time_lo (doubles), the outcome of the last propagation (int64_t), its number
 * of steps (uint64_t), min |h| and max |h| (doubles). Each integrator sends ONE packed block; the RCCL communicators are
 * created once per list of devices and kept. */
#define HY_GATHER_RESULT_ROWS 6
int hy_ensemble_gather_results(const hy_tab *tabs, size_t n, int dst_device, double *out, size_t out_words, int out_is_device,
                               int *used_rccl);

#ifdef __cplusplus
}
#endif

#endif
