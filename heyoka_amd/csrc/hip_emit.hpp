// HIP source generation for the batch Taylor stepper (gfx950 / CDNA4).
//
// Replaces the LLVM IR emission of the reference (taylor_add_adaptive_step(),
// src/taylor_00.cpp:712-865; taylor_compute_jet(), src/taylor_02.cpp:1307-1419; the per-node
// taylor_diff() rules under src/math/*.cpp) with generation of a HIP source module that is
// compiled at run time with hiprtc. One system per lane ("unrolled" mode) or one system per group
// of L lanes with the jets of the nonlinear sub-DAGs resident in registers ("cluster" mode).
#pragma once

#include <cstdint>
#include <array>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "decompose.hpp"
#include "kernel_args.hpp"

namespace heyoka_amd
{

enum class emit_mode { unrolled, cluster, table, block };

// Developer switches of the generators: experiments and the test matrix. ALL of them are read from the environment in ONE
// place, dev_switches::from_env() (hip_emit.cpp), when an integrator is constructed; the generators only see this struct.
//   HEYOKA_AMD_V5_EVENTS=0            stepper with events: not on the one-lane-per-pair kernel (lane-pair kernel instead)
//   HEYOKA_AMD_COMPACT_TC=0           stepper with events: full instead of compact Taylor coefficients
//   HEYOKA_AMD_NO_EVENTS_IN_STEPPER   event equations in a kernel of their own (hy_ev_jets) instead of inside the stepper
//   HEYOKA_AMD_NO_PAIR_EVENTS         close-encounter events through the generic statements, not on the lanes of their pairs
//   HEYOKA_AMD_NO_REFILL              one-lane-per-pair kernel: whole groups of systems from the queue, no per-system refill
//   HEYOKA_AMD_BLOCK_V2=0             block mode: generic cluster phase
//   HEYOKA_AMD_BLOCK_OPTS             block mode: items switched one by one, separated by ',' or ':' (the list: hip_emit_block_gen.hpp)
//   HEYOKA_AMD_NO_STATE_ALIASES       planner: no alias u variables for state variables in history position
//   HEYOKA_AMD_CLUSTER_V1             first-generation cluster generator
//   HEYOKA_AMD_MULTI_CLASS=0          planner: no multi-class plans (clusters of several shapes / levels)
//   HEYOKA_AMD_TABLE_LDS=0|1          table stepper: tape in HBM / in LDS (default: by size)
//   HEYOKA_AMD_STAGED_WPS=1|2|4       staged table stepper: wavefronts per system (default: by the size of the tape)
//   HEYOKA_AMD_EV_INLINE_MAX_NONLINEAR  budget of nonlinear nodes of the event equations inside the stepper
//   HEYOKA_AMD_V5_PRIO, HEYOKA_AMD_V5_OPTS, HEYOKA_AMD_V5_PAD   one-lane-per-pair kernel: issue priorities, round-5 items
//                                     switched off one by one (A/B harness), sensitivity padding (see hip_emit_cluster2_gen.hpp)
// (HEYOKA_AMD_EMIT_MODE, HEYOKA_AMD_ONE_LANE, HEYOKA_AMD_PAIR_SPLIT, HEYOKA_AMD_EVENTS_ON_CLUSTER map onto kwargs of the
// integrator - taylor_adaptive_batch.cpp -; HEYOKA_AMD_HIPRTC_FLAGS, HEYOKA_AMD_SCRATCH_GIB, HEYOKA_AMD_GATHER_RCCL and
// HEYOKA_AMD_EVENTS_TIMING belong to the runtime, not to code generation.)
struct dev_switches {
    bool v5_events = true, compact_tc = true, events_in_stepper = true, pair_events = true, refill = true, block_v2 = true,
         state_aliases = true, cluster_v1 = false, linearise = true, multi_class = true;
    int table_lds = -1, ev_inline_max_nonlinear = -1, v5_prio = 2, staged_wps = 0;
    // HEYOKA_AMD_UNROLLED_WAVES=n: the straight-line stepper is compiled for n wavefronts per SIMD (amdgpu_waves_per_eu: the
    // register allocator gets 512 / n registers per lane and spills the rest - the two-wavefront experiment of round 5).
    int unrolled_waves = 0;
    // Straight-line stepper with register-resident jets (see emit_unrolled_kernel(); A/B: profiles/r06_two_body_unrolled_ab.log):
    // literal-zero coefficients folded in the generator and the Horner steps over leading zeros collapsed into one
    // (HEYOKA_AMD_UNROLLED_TRIM=0: off), one running sum for the sum of squares (HEYOKA_AMD_UNROLLED_MERGE_SSQ=0: off), the
    // coefficients of a variable which only defines x' = v re-derived from those of x (HEYOKA_AMD_UNROLLED_DERIVE=0: off).
    bool unrolled_trim = true, unrolled_merge_ssq = true, unrolled_derive = true;
    // Register-resident jets of the state variables up to this estimate of the doubles a lane keeps (reg_jet_estimate()).
    // (-1: automatic - 270 with the folded histories of the default arithmetic, 200 otherwise.)
    int reg_jets_max = -1;
    std::string v5_opts, v5_pad;
    // HEYOKA_AMD_BLOCK_OPTS: items of block mode switched one by one (A/B harness, timing experiments), separated by ',' or
    // ':'; emit_block() parses the string once (block_switches, hip_emit_block_gen.hpp: the list of the switches).
    std::string block_opts;
    static dev_switches from_env();
};

struct emit_options {
    dev_switches dev;
    std::uint32_t order = 20;
    bool high_accuracy = false;
    emit_mode mode = emit_mode::unrolled;
    std::uint32_t block_size = 256;
    // Number of systems integrated at the same time (0: unknown); steers latency- vs throughput-oriented variants.
    std::uint64_t batch_size = 0;
    // Wave-cluster steppers: emit the stepper of an integrator with events - every launch is a mode-4 step (jets of the
    // state variables to a.tc, selector norms to a.sel_norms, no state update; emitted_module::cluster_mode4).
    bool event_stepper = false;
    // Wave-cluster generator (kw::cluster_kernel / hy_tab_config::cluster_kernel): 0 = automatic - the first one which
    // applies out of 5 (one lane per pair cluster, two wavefronts per SIMD), 3 (lane pairs), 2 (one lane per cluster,
    // pipelined orders), 1 (first generation) -, otherwise the search starts at the given generator.
    int cluster_kernel = 0;
    // Correctly rounded quotients in the recurrences of the pair kernels (division by the order, quotient of the pow
    // recurrence) instead of the reciprocal forms (within 1 ulp of them): kw::exact_division.
    bool exact_division = false;
    // Order of the additions inside the convolutions of the straight-line (unrolled) generator: 0 automatic = 2; 1 = the
    // reference's default mode (products first, pairwise sum: src/math/prod.cpp:386-395), 2 = the reference's compact mode
    // (running sum from 0: src/math/prod.cpp:686-698; one FMA per term). kw::sum_order. The table stepper always uses the
    // running sums, the cluster kernels their own FMA chains.
    int sum_order = 0;
    // Decompositions the wave-cluster / block planners cannot shape: straight-line code up to this many nodes, the
    // table-driven steppers beyond (kw::compact_mode lowers it: short compile times).
    std::uint32_t unroll_max_nodes = 150;
    // Block mode: linear nodes fed by one cluster stay glue nodes (plan_limits::absorb_linear off) - the internal program whose
    // scalings were moved out of the clusters for the v2 cluster phase (externalise_scalings()).
    bool block_no_absorb = false;
    // emit_event_jets() and the kernels of dense_output_text.hpp: the stepper they accompany leaves out the Taylor coefficients
    // of order >= 1 of the state variables defined by another state variable (emitted_module::compact_tc): read them as
    // parent^[k-1] / k.
    bool compact_tc = false;
    // Stepper with events on the one-lane-per-pair kernel: the decomposition of the system WITH the event equations
    // (prog.ev_u). When set, the stepper evaluates the event equations itself from
    // the jets of the state variables in LDS, extends the norms of the step-size selector to them, takes the final step
    // size and updates the state (emitted_module::events_in_stepper): hy_ev_jets and the dense-output pass over the Taylor
    // coefficients drop out of a step.
    const taylor_program *ev_prog = nullptr;
    // Number of TERMINAL events among the event equations of ev_prog (they come first). Without terminal events no step is
    // ever truncated, so nothing behind the stepper reads the Taylor coefficients of the state variables: they are stored
    // on request only (hy_kargs::pad bit 0; a later get_tc() regenerates them from the snapshot of the step).
    std::uint32_t n_t_events = 0;
    // callback::angle_reducer fused into the propagate kernel: sorted indices of the state variables which
    // are reduced to [0, 2 pi) right after every state update. Empty: no reduction, and not a byte of the source differs. Only
    // the straight-line, the table (both tape placements) and the first-generation / multi-class wave-cluster generators
    // implement it (emitted_module::angle_reduce_fused); the module is used for mode-1 launches only.
    std::vector<std::uint32_t> angle_reduce;
};

struct emitted_module {
    std::string source;
    std::string kernel_name; // step / propagate kernel
    std::string dout_name;   // dense-output kernel
    std::string tc_kernel_name; // optional variant of the stepper that writes the Taylor coefficients
    bool tc_optional = false;   // the main kernel works with a.tc == nullptr
    std::uint32_t block_size = 256;
    std::uint32_t lanes_per_system = 1;
    std::uint32_t n_clusters = 0; // cluster / block modes
    std::uint32_t lds_bytes = 0;
    emit_mode mode = emit_mode::unrolled;
    // Statistics (logged like the reference logs decomposition sizes).
    std::uint64_t n_statements = 0;
    std::string notes;
    // Which generation of the wave-cluster generators wrote the kernel: 0 = not a wave-cluster kernel, otherwise the numbers
    // of emit_options::cluster_kernel - 1 (first generation, multi-class), 2 (pipelined), 3 (lane pairs), 5 (one lane per
    // pair). The dispatch in emit_hip_module() reads this (and the refusal_code of an attempt which was refused), never the
    // prose of `notes`.
    int cluster_generation = 0;
    // Block mode: the cluster phase is the rolled "v2 cluster phase" (the pair phase, see hip_emit_block_pair.cpp).
    bool block_v2_phase = false;
    // Cluster mode: doubles of jet scratch needed per resident wave.
    std::uint64_t scratch_per_wave = 0;
    bool persistent = false;
    // Extra hiprtc options of the module (space separated), on top of the common ones.
    std::string compile_flags;
    // The stepper implements mode 4 in its cluster form (see hy_kargs::sel_norms).
    bool cluster_mode4 = false;
    // Mode 4 writes a COMPACT set of Taylor coefficients: for a state variable x defined by another state variable
    // (x' = v) only the order-0 row; x^[k] = v^[k-1] / k is left to the consumers (hy_dout_c and hy_tc_expand in the module
    // of emit_compact_tc_module(), with hy_ev_jets in the one of emit_event_jets()): half of the 6 KB per system of an N-body
    // ensemble never travel.
    bool compact_tc = false;
    // Mode 4 also evaluates the event equations, takes the final step size and updates the state (emit_options::ev_prog).
    bool events_in_stepper = false;
    // Single-step launches (mode 0) understand hy_kargs::pad bit 2: a.tfin_hi[] holds a time per system, and the Taylor
    // coefficients of a step are stored only if the step reaches it (or has length zero). The lock-step loop of
    // propagate_grid() passes the next grid time of every system: 6 GB of coefficients per sweep of 1 048 576 outer Solar
    // Systems otherwise, for dense output which a handful of steps need.
    bool tc_by_threshold = false;
    // Propagate-mode launches (mode 1) understand hy_kargs::pad bit 2 as well: see hy_kargs::tc_thr.
    bool grid_multi_step = false;
    // When the code was generated from a rewritten INTERNAL program (state-variable aliases, padded clusters, restored unit
    // scalings - the user-visible decomposition is never touched): its text, one node per line in the format of the
    // decomposition strings, then the definitions of the state derivatives. Lets the tests run the oracle's interpreter
    // on the rewritten program and check that the rewrites do not change a single bit of the jets.
    std::string internal_program;
    // The stepper reduces the state variables of emit_options::angle_reduce after every state update.
    bool angle_reduce_fused = false;
    // emit_mode::cluster ended on a generic stepper (straight-line or table): no wave-cluster / block planner could shape the
    // decomposition, `notes` says why ("cluster mode not applicable: ...").
    bool cluster_fallback = false;
};

// Why a generator or the planner refused a program: the diagnostic for the notes and the log, and - for the reasons the
// selection of the stepper reacts to - a code, so that nothing ever depends on the wording of the text.
//   not_isomorphic     the clusters have different shapes (cured by padding, unit scalings, private inputs, or by planning
//                      without the absorption of linear nodes)
//   too_many_clusters  more clusters than plan_limits::max_clusters (block mode takes over)
//   state_var_history  a state variable is a history operand of a nonlinear function (cured by alias u variables)
//   other              everything else: a reason nobody reacts to
enum class refusal_code { none, not_isomorphic, too_many_clusters, state_var_history, other };
struct emit_refusal {
    refusal_code code = refusal_code::none;
    std::string text; // the diagnostic
    emit_refusal() = default;
    emit_refusal(refusal_code c, std::string t) : code(c), text(std::move(t)) {}
    // (Implicit: the generators write `why_not = "...";`.)
    emit_refusal(std::string t) : code(t.empty() ? refusal_code::none : refusal_code::other), text(std::move(t)) {}
    emit_refusal(const char *t) : emit_refusal(std::string(t)) {}
    bool empty() const
    {
        return code == refusal_code::none;
    }
    void clear()
    {
        *this = emit_refusal{};
    }
};

// Textual form of a flattened program (see emitted_module::internal_program).
std::string program_to_string(const taylor_program &);

emitted_module emit_hip_module(const taylor_program &prog, const emit_options &opts);

// Companion of the wave-cluster steppers for integrators with events: kernel hy_ev_jets, one system per lane - the jets
// of the event equations from the jets of the state variables in a.tc (only the part of the decomposition the event
// equations depend on), the norms of the step-size selector extended to the event equations and the final step size.
// prog is the decomposition of the system *with* the event equations (prog.ev_u). Returns a module with an empty source
// (and the reason in why_not) when the event equations need too much of the decomposition. With emit_options::compact_tc
// the kernels of emit_compact_tc_module() come first in the module. (hip_emit_events.cpp)
emitted_module emit_event_jets(const taylor_program &prog, const emit_options &opts, std::string &why_not);

// The companion module of a stepper which stores compact Taylor coefficients (emit_options::compact_tc) and evaluates the
// event equations itself (emitted_module::events_in_stepper): only the kernels which serve the compact coefficients -
// hy_dout_c, the dense output (state update of a step with events), and hy_tc_expand, which fills in the rows the stepper
// left out for whoever reads the full array afterwards. (dense_output_text.cpp)
emitted_module emit_compact_tc_module(const taylor_program &prog, const emit_options &opts);

// Dense output over the ROWS of the event log (event_detection.hpp): hy_dout_rows evaluates the Taylor coefficients of
// the row's system at the row's root and fills the state columns of the row, with the operations and the operation
// order of hy_dout (full coefficients) or - emit_options::compact_tc - of hy_dout_c (the rows of the variables defined
// by another state variable are derived: x^[k] = v^[k-1] / k); rows of terminal events copy the state after the step.
// A module of its own, compiled only for integrators with recording callbacks. (dense_output_text.cpp)
std::string make_event_log_dout_source(const taylor_program &prog, const emit_options &opts);

// The same computation as straight-line statements for use INSIDE a stepper (the one-lane-per-pair kernel in mode 4): sv(i, k)
// gives the expression of the order-k coefficient of state variable i (every use of a coefficient goes through ONE
// definition: one LDS read), ev_store(event, k, value) the statement which publishes a coefficient of an event equation.
// Appends the statements to `out` and returns, per event equation, the names of its coefficients by order (for the norms
// of the step-size selector and the exclusion test). Returns false (and the reason) if the event equations depend on
// too much of the decomposition or on functions defined through node rules.
// Lanes of a system as a vector unit for ISOMORPHIC terms of a sum (optional): the event equations of N-body problems are
// sums of a few terms of one shape - (x_1 - x_2)^2 + (y_1 - y_2)^2 + (z_1 - z_2)^2, x vx + y vy + z vz - whose convolutions
// dominate the cost. With these hooks the terms of such a sum are evaluated ONCE, term c by lane c of the system (leaf
// position p of the shared shape reads the state variable leaf_vars[p][c]), and the sum collects them with lane broadcasts
// in the order of its arguments - the same operations on the same operands as the term-by-term evaluation, bit for bit.
struct ev_lane_hooks {
    // Access class of a state variable (variables of one class are read by the same expression up to an offset).
    std::function<int(std::uint32_t)> sv_class;
    // Coefficient k of the state variable which THIS lane holds at leaf position p (class cls).
    std::function<std::string(std::uint32_t p, std::uint32_t k, int cls)> sv_lane;
    // Value of v in lane c of the system.
    std::function<std::string(const std::string &v, std::uint32_t c)> lane_bcast;
    std::uint32_t max_terms = 4;
    // Out: per leaf position the state variable of term c (c < number of terms of the sum, <= max_terms), and its class.
    std::vector<std::vector<std::uint32_t>> leaf_vars;
    std::vector<int> leaf_class;
};

// skip_events (optional, one flag per event equation): event equations which the caller evaluates by other means - their
// entry of ev_coeffs stays empty and the nodes only they depend on are not generated. (hip_emit_events.cpp)
bool emit_event_jets_inline(const taylor_program &prog, const emit_options &opts,
                            const std::function<std::string(std::uint32_t, std::uint32_t)> &sv,
                            const std::function<std::string(std::uint32_t, std::uint32_t, const std::string &)> &ev_store,
                            std::string &out, std::vector<std::vector<std::string>> &ev_coeffs, std::string &why_not,
                            ev_lane_hooks *lanes = nullptr, const std::vector<char> *skip_events = nullptr);

// Is the event equation u (a u variable of prog) a squared distance plus a constant,
//     +-((a_0 - b_0)^2 + (a_1 - b_1)^2 + (a_2 - b_2)^2) + c,        a_i, b_i state variables,
// written with products, pow(., 2) or sum_sq and sums / differences in any nesting? The close-encounter events of an
// N-body problem have this form - and the pair kernels hold the Taylor coefficients of exactly these squared distances.
// (hip_emit_events.cpp)
struct pair_distance_event {
    std::array<std::pair<std::uint32_t, std::uint32_t>, 3> diffs; // (a_i, b_i), state variable indices
    double c = 0;
    double sign = 1; // -1: the squares are subtracted, c - |r_i - r_j|^2
};
bool match_pair_distance_event(const taylor_program &prog, std::uint32_t u, pair_distance_event &out);

// callback::angle_reducer on the device. angle_reduce_helper_source: the __device__ function hy_angle_red(x) =
// x - twopi * floor(x / twopi), twopi = 0x1.921fb54442d18p+2, with a rounded quotient, a rounded product and a rounded
// difference (no FMA contraction), non-finite x returned as it is - the ONE definition which the stand-alone kernel and the
// fused steppers share. make_angle_reduce_source(): module of the stand-alone kernel hy_angle_reduce (one thread per
// (flagged variable, system) over the device-resident state). emit_angle_reduce_variant(): the stepper of `prog` with the
// reduction of opts.angle_reduce fused in, or a module with an empty source and the reason in why_not when the generator
// which serves prog does not implement it. angle_reduce_host(): the same arithmetic on the host.
extern const char *const angle_reduce_helper_source;
std::string make_angle_reduce_source();
emitted_module emit_angle_reduce_variant(const taylor_program &prog, const emit_options &opts, std::string &why_not);
double angle_reduce_host(double x) noexcept;

// Format a double as a C++17 hexadecimal floating-point literal (exact round trip).
std::string fp_literal(double);

} // namespace heyoka_amd
