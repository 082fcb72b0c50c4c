// The argument blocks of the kernels. Every kernel takes ONE struct by value; the host fills the struct and the device
// source declares it, and both come from the one field list written here: HY_KARGS(host, dev, fields) defines the host
// struct `host` and the function host_text(), the text "struct dev { fields };" which the generators put into the HIP
// source - one declaration per line, without the comments (the preprocessor drops them) and without the default
// initialisers of the host. u64 / i64 are the typedefs of the device prelude (emit_detail::prelude()); the blocks of the
// modules without the prelude spell the types out.
//
// A new block: one HY_KARGS() below, one entry in HY_KARGS_BLOCKS at the end of the file (tests/test_kernel_args.py then
// compiles an empty kernel over the text and compares the size of its argument segment with sizeof of the host struct).
#pragma once

#include <string>
#include <string_view>

namespace heyoka_amd
{

using u64 = unsigned long long;
using i64 = long long;

namespace detail
{

// The declarations of a stringified field list, each one between `before` and `after`, without its initialiser.
inline std::string kargs_fields(std::string_view fields, const char *before, const char *after)
{
    std::string ret;
    for (std::size_t b = 0, e = 0; (e = fields.find(';', b)) != std::string_view::npos; b = e + 1u) {
        const auto decl = fields.substr(b, e - b);
        const auto first = decl.find_first_not_of(' ');
        ret += before + std::string(decl.substr(first, decl.find(" = ") - first)) + after;
    }
    return ret;
}

} // namespace detail

} // namespace heyoka_amd

#define HY_KARGS(host, dev, ...)                                                                                               \
    struct host {                                                                                                              \
        __VA_ARGS__                                                                                                            \
    };                                                                                                                         \
    inline std::string host##_text()                                                                                           \
    {                                                                                                                          \
        return "struct " #dev " {\n" + detail::kargs_fields(#__VA_ARGS__, "    ", ";\n") + "};\n";                             \
    }                                                                                                                          \
    inline std::string host##_parameters()                                                                                     \
    {                                                                                                                          \
        const auto s = detail::kargs_fields(#__VA_ARGS__, "", ", ");                                                           \
        return s.substr(0, s.size() - 2u);                                                                                     \
    }

namespace heyoka_amd
{

// The steppers (hy_taylor, hy_taylor_tc, hy_ev_jets).
HY_KARGS(hy_kargs, hy_kargs,
    double *state;            // [n_eq * N] rw
    const double *pars;       // [n_par * N]
    double *time_hi;          // [N] rw
    double *time_lo;          // [N] rw
    const double *lim;        // step mode: signed max step [N]; propagate mode: max_delta_t > 0 [N] or null
    const double *tfin_hi;    // propagate mode: final times (double-length) [N]
    const double *tfin_lo;    // [N]
    double *last_h;           // [N] out
    i64 *outcome;             // [N] out (taylor_outcome)
    double *min_h;            // [N] out (propagate mode)
    double *max_h;            // [N] out (propagate mode)
    u64 *n_steps;             // [N] out (propagate mode)
    double *tc;               // [n_eq * (order + 1) * N] jet scratch == Taylor coefficients output
    u64 N;                    // number of systems
    u64 max_steps;            // propagate mode: 0 = unlimited
    int mode;                 // 0 = single step, 1 = propagate_until, 2 = raw step, 4 = step with events
    // Stepper with events which evaluates the event equations itself (emitted_module::events_in_stepper): bit 0 = every
    // workgroup stores its Taylor coefficients (otherwise only those in which an event is possible), bit 1 = store NOTHING
    // but the coefficients (the launch which regenerates them from the snapshot of the state before the step). 0 elsewhere.
    int pad;
    unsigned int *counters;   // [16] device counters: [0] lanes with non-finite state, [1] work-queue head
    double *scratch;          // cluster mode: jet scratch, scratch_per_wave doubles per resident wave
    double tfin_s_hi, tfin_s_lo; // propagate mode, scalar final time (used when tfin_hi == nullptr)
    // mode 4 (stepper with events, no state update): Taylor coefficients of the event equations
    // [(event * (order + 1) + k) * N + system] and max_i |x_i| per system.
    double *ev_tc;
    double *max_abs_state;
    // mode 4 on the wave-cluster steppers (jets of the state variables to tc, no state update): the three norms of the
    // step-size selector over the state variables, [3 * N] = max |x^[0]|, max |x^[p]|, max |x^[p-1]| per system. The
    // jets of the event equations and the final step size are computed from tc by hy_ev_jets (emit_event_jets()).
    // (With the event equations inside the stepper the first N entries carry its verdict per system for the detection
    // kernel instead: 0.0 = no event possible in this step.)
    double *sel_norms;
    // Taylor coefficients on demand (hy_kargs::pad bit 2, emitted_module::tc_by_threshold / grid_multi_step): a time per
    // system - the next grid point of propagate_grid() -; a step stores its coefficients only if it reaches that time, and in
    // propagate mode (mode 1) the system leaves the step loop after that step: one launch takes every system from one grid
    // point to the next instead of one step further.
    const double *tc_thr;
    // ... and, out, per system: 1.0 if its last step was clamped to the remaining time (h == rem.hi: the system has reached
    // its final time - the post-step kernel of propagate_grid() then treats it as done), 0.0 otherwise.
    double *grid_done;
)

namespace detail
{

// hy_dout, the dense-output kernel of every stepper module (emit_dout(), dense_output_text.cpp). The kernel takes the fields one by one: its
// parameter list is dout_kargs_parameters().
HY_KARGS(dout_kargs, hy_dout_args,
    double *out;              // [n_eq * N]
    const double *tc;
    const double *hs;         // [N] time from the beginning of the step
    u64 N;
)

// The post-step kernels (hy_grid_post / hy_until_post / hy_grid_unsample / hy_indep_override, see make_grid_source()).
// The call sites name the fields they set; the others keep the null / zero below.
HY_KARGS(grid_kargs, hy_grid_args,
    const double *grid = nullptr;
    double *out = nullptr;
    const double *tc = nullptr;
    const double *thi = nullptr;
    const double *tlo = nullptr;
    const double *last_h = nullptr;
    const i64 *outcome = nullptr;
    double *rem_hi = nullptr;
    double *rem_lo = nullptr;
    const double *mdt = nullptr;
    const int *t_dir = nullptr;
    double *lim = nullptr;
    unsigned *gidx = nullptr;
    double *min_h = nullptr;
    double *max_h = nullptr;
    u64 *n_steps = nullptr;
    unsigned *counters = nullptr;
    u64 N = 0;
    unsigned n_grid = 0;
    // (Next grid time of every lane, +-inf once the lane is through its grid: hy_kargs::pad bit 2 of the next sweep.)
    double *next_tg = nullptr;
    // Launches which take every lane from one grid point to the next (emitted_module::grid_multi_step): the stepper leaves
    // the counters / extrema of ITS launch in n_steps / min_h / max_h, which are accumulated here (null: single-step sweeps).
    u64 *acc_n_steps = nullptr;
    double *acc_min_h = nullptr;
    double *acc_max_h = nullptr;
    // (... and whether the lane's last step was clamped to its remaining time: hy_kargs::grid_done.)
    const double *grid_done = nullptr;
    // (... and the stepper's count of systems which went non-finite in the launch, hy_kargs::counters[0]; nonzero with the
    // reference's semantics: the launch is rolled back, nothing is recorded - counters[3] = 1 tells the host. Null: no check.)
    const unsigned *launch_nf = nullptr;
    // (The grid index of every lane before this sweep's samples: hy_grid_unsample takes them back. Null: not kept.)
    unsigned *gidx_prev = nullptr;
    // Independent semantics (config::batch_semantics == 3), null / 0 otherwise. retired[N]: the sticky outcome of a system
    // retired in this call (0: not retired); outcome_w: the outcome array, writable - the sticky outcome is put back after
    // every zero-length step; counters[4] / [5] count the systems retired by events / as non-finite. override_oc:
    // hy_indep_override only - the outcome (step_limit, cb_stop) of the systems which are neither done nor retired.
    i64 *retired = nullptr;
    i64 *outcome_w = nullptr;
    i64 override_oc = 0;
    // (... and the cooldown flags / durations of the terminal events, [n_te * N]: see hy_indep_retired(). Null: none.)
    int *cd_active = nullptr;
    const double *cd_second = nullptr;
    // Grid observables (make_grid_source() with a section), null otherwise: the parameters [n_par * N], the
    // staging buffer of one sample [dim * N] (staged mode only) and, for hy_grid_obs0, the current state [dim * N].
    const double *pars = nullptr;
    double *stage = nullptr;
    const double *state = nullptr;
)

// hy_ev_stop (make_grid_source()).
HY_KARGS(ev_stop_kargs, hy_ev_stop_args,
    i64 *outcome;
    const int *te_stop;
    u64 N;
    unsigned n_te, pad;
)

// hy_dout_c, hy_tc_expand (emit_compact_tc_module(), dense_output_text.cpp). hfull != nullptr: only the lanes whose step was truncated - hs[s] !=
// hfull[s] - are updated: the stepper which evaluates the event equations itself has already taken the full step
// everywhere.
HY_KARGS(doutc_kargs, hy_doutc_args,
    double *out;
    const double *tc;
    const double *hs;
    u64 N;
    const double *hfull;
)

// hy_dout_rows (make_event_log_dout_source(), dense_output_text.cpp). n_rows != nullptr: the number of rows of the step is read from the device
// (written by hy_evr_scan), n_max bounds it.
// hy_obs_rows (make_event_log_obs_source(), event-log observables) takes the same block and reads its last two fields: the
// parameters [n_par * N] and, staged mode only, the samples of the rows of the step [n_reads * n_max]; null for hy_dout_rows.
HY_KARGS(drow_kargs, hy_drow_args,
    double *rows;
    const double *tc;
    const double *state;
    const u64 *n_rows;
    u64 n_max;
    u64 N;
    unsigned row_doubles, pad;
    const double *pars;
    double *stage;
)

// hy_copy_arrays (make_event_detection_source()).
HY_KARGS(copy_kargs, hy_copy_args,
    double *dst[4];
    const double *src[4];
    u64 n[4];
)

// hy_angle_reduce (make_angle_reduce_source()).
HY_KARGS(ar_kargs, hy_ar_kargs,
    double *state;            // [n_eq * N]
    const unsigned *idx;      // [n_idx] state variables to reduce
    unsigned long long N;     // number of systems
    unsigned n_idx;
)

// hy_detect_events (event_detection.hpp).
HY_KARGS(ed_kargs, hy_ed_args,
    const double *ev_tc;      // [(event * (order + 1) + k) * N + lane], terminal events first
    const double *h;          // [N] step taken
    const double *g_eps;      // [N]
    const int *dirs;          // [n_te + n_nte]
    const double *cd_first;   // [n_te * N] terminal-event cooldowns (valid if cd_active != 0)
    const double *cd_second;  // [n_te * N]
    const int *cd_active;     // [n_te * N]
    double *out;              // [2][N][ed_max_detected()][4]: idx, root, d_sgn, abs_der
    unsigned *counts;         // [2][N]
    unsigned *flags;          // [0] root isolations which failed, [1] event lists which overflowed, [2] root findings which
                              // failed (event, lane) - the reference logs a warning and ignores the event
    u64 N;
    unsigned n_te, n_nte;
    // Device-side error bound of the Taylor series of the event equations (src/taylor_adaptive_batch.cpp:744-767):
    // when mas != nullptr, g_eps is computed from max |x_i| and the tolerance and written to g_eps_out.
    const double *mas;
    double *g_eps_out;
    double tol;
    double *wl;               // working lists of the root isolation, ed_work_list_bytes_per_slot() per launched thread
    u64 wl_slots;             // number of launched threads (grid-stride loop over the lanes)
    // Optional [N]: 0.0 for the lanes in which the stepper has already ruled out events in this step (its conservative
    // exclusion test on the jets it computed, emitted_module::events_in_stepper): they are skipped without reading their
    // event jets.
    const double *maybe;
)

// Per-lane bookkeeping of a step with events on the device (src/taylor_adaptive_batch.cpp:771-1030): hy_ev_pre
// (truncation of the step at the first terminal event, size of the record buffer), the dense-output kernel, hy_ev_post
// (time update, non-finite check, cooldown update, outcomes, compaction of the lanes with events into records),
// hy_ev_scatter (cooldowns / outcomes set by the host for the lanes whose terminal events triggered).
// Record of a lane with events: 8 doubles (lane, n_te, n_nte, g_eps, h, new time hi, new time lo, 0) followed by
// 4 doubles per event (idx, root, d_sgn, |derivative|), terminal events first, in detection order.
HY_KARGS(ep_kargs, hy_ep_args,
    const double *h;          // [N] step sizes of the stepper
    const double *ed_out;
    const unsigned *counts;
    double *dout_h;           // [N] final step sizes
    const double *g_eps;      // [N]
    const double *state;      // [dim * N], after the update
    double *time_hi, *time_lo;
    const double *lim;
    double *cd_first, *cd_second;
    int *cd_active;
    i64 *outcome;
    double *last_h;
    double *rec;
    u64 *cursor;              // [0] record doubles needed (hy_ev_pre), [1] record doubles written (hy_ev_post)
    const double *upd;        // hy_ev_scatter: n_cd x (position, first, second) then n_oc x (lane, outcome)
    u64 N;
    unsigned n_te, n_nte, dim, n_cd, n_oc, pad;
    // Every callback is the library's counting callback (core_*_event::native_counter): hy_ev_post applies the events of
    // a lane itself - counts per event in ev_counts[n_te + n_nte] (terminal events first), cooldown and outcome of the
    // first terminal event, cooldown settings in te_cd[n_te] (< 0: deduced) - and writes no records.
    int native;
    u64 *ev_counts;
    const double *te_cd;
)

// hy_evr_count / hy_evr_scan / hy_evr_write, the kernels of the event log (make_event_recorder_source()).
HY_KARGS(evr_kargs, hy_evr_args,
    const double *ed_out;      // as ed_kargs::out
    const unsigned *counts;    // as ed_kargs::counts
    const double *dout_h;      // [N] final step sizes
    const double *time_hi, *time_lo; // [N] after hy_ev_post
    const i64 *outcome;        // [N] after hy_ev_post / hy_ev_native
    const int *is_rec;         // [n_te + n_nte] != 0: the event has a recording callback (terminal events first)
    unsigned *lane_rows;       // [N] rows of the lane in this step
    u64 *blk;                  // [ceil(N / 256)] sums per workgroup, then (after hy_evr_scan) their exclusive scan
    u64 *total;                // [0] rows of this step
    double *rows;              // first new row of the log
    u64 N;
    unsigned n_te, n_nte, row_doubles, pad;
)

// hy_ev_action. The kernel serves the systems [first, first + count). force < 0: a system is served if outcome[i] is the
// index of a terminal event with an action (the continuing outcome hy_ev_native wrote), by that event's section;
// force >= 0: every system of the range is served by the section of the terminal event `force` (the host loop of a mixed
// integrator, one system at a time).
HY_KARGS(eva_kargs, hy_eva_args,
    const i64 *outcome;
    double *state;
    const double *pars;
    const double *time_hi;
    u64 N, first, count;
    i64 force;
)

// hy_step_action. counter: the number of systems whose condition held (one atomic per wavefront; null without a
// condition). retired / outcome_w / lim (/ gidx, n_grid in propagate_grid()): the arrays of the independent semantics,
// null otherwise.
HY_KARGS(sa_kargs, hy_sa_args,
    const double *last_h;
    double *state;
    const double *pars;
    const double *time_hi;
    unsigned *counter;
    i64 *retired;
    i64 *outcome_w;
    double *lim;
    unsigned *gidx;
    u64 N;
    unsigned n_grid, pad;
)

// hy_tmap / hy_tmap_cloud (make_taylor_map_source()).
HY_KARGS(tmap_kargs, hy_tmap_args,
    const double *state; // [dim * N] SoA state of the variational integrator
    const double *in;    // [n_args * N]
    double *out;         // [n_orig * N]
    unsigned long long N;
)
HY_KARGS(tmap_cloud_kargs, hy_tmap_cloud_args,
    const double *state;
    const double *delta; // [N * n_args * n_samples], or [n_args * n_samples] when shared
    double *out;         // [N * n_orig * n_samples]
    unsigned long long N, n_samples;
    unsigned blocks_per_sys, shared;
)

// hy_cfunc (cfunc.cpp).
HY_KARGS(cf_kargs, hy_cf_args,
    double *out;
    const double *in;
    const double *pars;
    const double *tm;
    u64 n;
)

// hy_c_out (make_cout_source()).
HY_KARGS(cout_kargs, hy_cout_args,
    double *out;
    const double *tm;
    const double *const *tcs;
    const double *thi;
    const double *tlo;
    u64 N;
    unsigned n_times;
    unsigned scalar_tm;
    double tm_s;
)

} // namespace detail

} // namespace heyoka_amd

// Every block, as X(host struct, device struct) with the host struct as seen from namespace heyoka_amd::detail. A new
// block is added here.
#define HY_KARGS_BLOCKS(X)                                                                                                     \
    X(hy_kargs, hy_kargs)                                                                                                      \
    X(dout_kargs, hy_dout_args)                                                                                                \
    X(grid_kargs, hy_grid_args)                                                                                                \
    X(ev_stop_kargs, hy_ev_stop_args)                                                                                          \
    X(doutc_kargs, hy_doutc_args)                                                                                              \
    X(drow_kargs, hy_drow_args)                                                                                                \
    X(copy_kargs, hy_copy_args)                                                                                                \
    X(ar_kargs, hy_ar_kargs)                                                                                                   \
    X(ed_kargs, hy_ed_args)                                                                                                    \
    X(ep_kargs, hy_ep_args)                                                                                                    \
    X(evr_kargs, hy_evr_args)                                                                                                  \
    X(eva_kargs, hy_eva_args)                                                                                                  \
    X(sa_kargs, hy_sa_args)                                                                                                    \
    X(tmap_kargs, hy_tmap_args)                                                                                                \
    X(tmap_cloud_kargs, hy_tmap_cloud_args)                                                                                    \
    X(cf_kargs, hy_cf_args)                                                                                                    \
    X(cout_kargs, hy_cout_args)
