// Private state of the host driver of the MI355X batch Taylor integrator (tab_core::impl): shared by taylor_adaptive_batch.cpp, tab_events.cpp, tab_propagate.cpp and grid_post.cpp.
#ifndef HEYOKA_AMD_TAB_IMPL_HPP
#define HEYOKA_AMD_TAB_IMPL_HPP

#include "logging.hpp"
#include "taylor_adaptive_batch.hpp"

#include <algorithm>
#include <array>
#include <cassert>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>

#include "dfloat.hpp"
#include "event_observables.hpp"
#include "hip_backend.hpp"
#include "hip_emit.hpp"
#include "grid_observables.hpp"
#include "hip_emit_detail.hpp"
#include "kernel_args.hpp"
#include "step_action.hpp"

namespace heyoka_amd::detail
{

// Shortest representation which round-trips, like the reference's fmt::format("{}", x) (fp_to_string(),
// src/detail/string_conv.cpp:64-80).
inline std::string fp_to_string(double x)
{
    char buf[64];
    const auto res = std::to_chars(buf, buf + sizeof(buf), x);
    return std::string(buf, res.ptr);
}

// Sets a value for the lifetime of the object and puts the previous one back.
template <typename T>
struct scoped_value {
    T &ref;
    T old;
    scoped_value(T &r, T v) : ref(r), old(r)
    {
        ref = v;
    }
    scoped_value(const scoped_value &) = delete;
    ~scoped_value()
    {
        ref = old;
    }
};

// The module of a generated section inside an integrator: its HIP source, the compiled code object (it lives in the
// process-wide cache) and the module loaded on the integrator's device at the first launch.
struct section_module {
    std::string source;
    std::shared_ptr<const compiled_module> cm;
    std::unique_ptr<aux_module> dm;

    aux_module &loaded(int device)
    {
        if (!dm) {
            dm = std::make_unique<aux_module>(cm, device);
        }
        return *dm;
    }
};

// The entry of key in a map of section modules; on first use make(entry) checks the section against the system and
// generates the source, which is compiled here. Nothing is ever dropped: a copy of the integrator starts with empty maps.
template <typename M, typename F>
typename M::mapped_type &find_or_build(M &map, const std::string &key, const char *label, const F &make)
{
    auto it = map.find(key);
    if (it == map.end()) {
        typename M::mapped_type v;
        make(v);
        const stopwatch sw;
        v.cm = hiprtc_compile_source(v.source);
        log_message(log_level::trace, std::string(label) + ": kernel compilation runtime: " + sw.str());
        it = map.emplace(key, std::move(v)).first;
    }
    return it->second;
}

struct tab_core::impl {
    sys_t sys;
    taylor_dc_t dc;
    taylor_program prog;
    std::uint32_t order = 0;
    double tol = 0;
    bool high_accuracy = false;
    bool compact_mode = false;
    // MI355X extensions of the configuration (tab_core::config): code generator, cluster generator, exact divisions,
    // steppers used with events, outcome semantics of propagate_for / propagate_until.
    int emitter = 0, cluster_kernel = 0, events_on_cluster = 0, batch_semantics = 0, sum_order = 0;
    bool exact_division = false;
    std::uint32_t N = 0; // batch size == number of systems.
    std::uint32_t dim = 0;
    int device = 0;

    emitted_module emitted;
    std::shared_ptr<const compiled_module> cmod;

    // Host mirrors (mutable: refreshed lazily from const getters).
    mutable std::vector<double> state, pars, time_hi, time_lo, tc, last_h, d_out;
    mutable std::vector<std::tuple<taylor_outcome, double>> step_res;
    mutable std::vector<std::tuple<taylor_outcome, double, double, std::size_t>> prop_res;

    // Device side (created lazily at the first operation needing the GPU).
    mutable std::unique_ptr<device_module> dmod;
    mutable device_buffer d_state, d_pars, d_thi, d_tlo, d_lim, d_tfhi, d_tflo, d_lasth, d_outcome, d_minh, d_maxh,
        d_nsteps, d_tc, d_counters, d_dout, d_douth;
    mutable void *stream = nullptr;

    // Synchronisation state.
    mutable bool host_newer = true;      // state/pars/time on the host must be uploaded.
    mutable bool dev_newer = false;      // state/time on the device must be downloaded.
    mutable bool tc_dev_newer = false;   // tc on the device is newer than the host mirror.
    mutable bool lasth_dev_newer = false;
    mutable bool step_res_dev_newer = false;
    mutable bool prop_res_dev_newer = false;
    bool sticky_host_ptr = false; // a mutable host pointer was handed out: sync eagerly.
    // The C++ interface handed out a reference / pointer to the host mirror of the state or of the times (the
    // reference's getters return references to members which every step updates in place, and its own benchmark keeps
    // one across steps: benchmark/outer_ss_long_term_batch.cpp, `const auto &times_v = ta.get_time()`): the mirrors are
    // refreshed after every kernel from then on.
    mutable bool sticky_const_refs = false;
    mutable bool sticky_time_refs = false; // (a reference to the times only: the state stays on the device)
    // Stepper with events on the wave-cluster kernels: the Taylor coefficients of order >= 1 of the state variables defined
    // by another state variable are not written by the stepper (emitted_module::compact_tc); hy_tc_expand fills them in
    // before anybody reads the full array.
    mutable bool tc_expand_pending = false;
    void ensure_tc_expanded() const;
    // Stepper with events which evaluates the event equations itself (emitted_module::events_in_stepper): the Taylor
    // coefficients of a step are stored only for the workgroups in which an event may have happened; the state and time
    // before the step are kept, and whoever reads coefficients which were not stored (get_tc(), update_d_output(),
    // continuous output, propagate_grid()) triggers a second launch of the stepper on the snapshot which stores nothing
    // but them (bit-identical: the same kernel on the same input). ev_all_tc: store them in every step (lock-step loops
    // which consume them step by step).
    device_buffer evs_state, evs_thi, evs_tlo, evs_pars;
    // Accounting of the steps with events (tab_core::set_event_timing() / get_event_stats(); bench.py's events leg): number
    // of steps, wall-clock ms of the five phases (only with the timing switched on: a stream synchronisation after each
    // phase), regeneration launches of the Taylor coefficients, systems which reported events.
    bool ev_timing = false;
    double ev_ms[5] = {0, 0, 0, 0, 0};
    std::uint64_t ev_steps = 0, ev_systems = 0;
    mutable std::uint64_t tc_regens = 0;
    mutable bool tc_partial = false;
    // propagate_grid() with Taylor coefficients on demand (emitted_module::tc_by_threshold) which was interrupted by a
    // non-finite state: d_tc mixes the coefficients of different steps. Cleared by the next step which stores them.
    mutable bool tc_stale = false;
    void check_tc_not_stale() const
    {
        if (tc_stale) {
            throw std::runtime_error("The Taylor coefficients of the last step are not available: the last propagate_grid() "
                                     "stored them on demand and was interrupted by a non-finite state");
        }
    }
    bool ev_all_tc = false;
    // (A caller who read the coefficients of the previous step - a step callback with dense output, say - will probably read
    // those of the next one: that step stores them all instead of paying for a second launch again.)
    mutable bool tc_regenerated = false;
    void ensure_tc_complete() const;
    std::uint64_t last_total_steps = 0;
    // Set by the lock-step propagate loop to override the device outcomes.
    mutable std::optional<taylor_outcome> prop_res_override;
    // Reference outcome semantics on the device-resident propagation (config::batch_semantics == 0): snapshot of the
    // state / times taken before the launch (a batch in which a lane goes non-finite is rolled back and re-run through
    // the lock-step loop: src/taylor_adaptive_batch.cpp:1404-1407, :1462-1467) and the flag which makes a step-limited
    // batch report step_limit in every lane (:1516) when its results are fetched.
    mutable device_buffer snap_state, snap_thi, snap_tlo;
    mutable bool fix_step_limit = false;
    bool force_lockstep = false;
    // ---- callback::angle_reducer ----
    // Options the stepper was generated with, and the stepper variants with a fused reduction, keyed by the sorted list of
    // reduced state variables: generated and compiled on first use (the compiled code objects live in the process-wide,
    // reference-counted caches of hip_backend.cpp like every other module), or the reason why the generator declined.
    emit_options eo;
    struct ar_variant {
        emitted_module em;
        std::shared_ptr<const compiled_module> cm;
        std::unique_ptr<device_module> dm;
        std::string why_not;
    };
    std::map<std::vector<std::uint32_t>, ar_variant> ar_variants;
    double ar_compile_seconds = 0;
    // Stand-alone kernel hy_angle_reduce and the index list it last ran with.
    mutable std::unique_ptr<aux_module> ar_mod;
    device_buffer d_ar_idx;
    std::vector<std::uint32_t> ar_idx_dev;
    // The callback of the running propagate_*() is a pure angle_reducer (set); how the callback of the last one ran.
    bool cb_is_reducer = false;
    int last_cb_path = 0;
    // ---- step_action (step_action.hpp) ----
    // The modules of the actions this integrator has met, keyed by the text of the action: checked against the system,
    // generated and compiled on first use (the code objects live in the process-wide cache), loaded at the first launch.
    struct sa_module : section_module {
        step_action_section sec;
    };
    std::map<std::string, sa_module> sa_modules;
    sa_module &get_sa_module(const step_action &act)
    {
        return find_or_build(sa_modules, act.to_string(), "step_action", [&](sa_module &v) {
            v.sec = make_step_action_section(act, state_variables_of(sys), prog.n_par);
            v.source = make_step_action_source(v.sec);
        });
    }
    // The counter of the stop condition; systems retired by it in the running / last sweep loop; the grid indices of the
    // running propagate_grid() loop (a system retired by the action is through its grid); every member of the callback of
    // the running propagate_*() is library-side, with at least one action; accounting of the timed launches.
    device_buffer d_sa_cnt;
    std::uint64_t n_stopped_by_action = 0;
    unsigned *sa_gidx = nullptr;
    unsigned sa_n_grid = 0;
    bool cb_is_library = false;
    double sa_ms = 0;
    std::uint64_t sa_timed = 0;
    ar_variant &get_ar_variant(const std::vector<std::uint32_t> &idx)
    {
        auto it = ar_variants.find(idx);
        if (it == ar_variants.end()) {
            ar_variant v;
            auto o = eo;
            o.angle_reduce = idx;
            v.em = emit_angle_reduce_variant(prog, o, v.why_not);
            if (!v.em.source.empty()) {
                const detail::stopwatch sw;
                v.cm = hiprtc_compile(v.em);
                ar_compile_seconds = v.cm->compile_seconds;
                detail::log_message(log_level::trace, "angle_reducer: stepper variant compilation runtime: " + sw.str());
            }
            it = ar_variants.emplace(idx, std::move(v)).first;
        }
        return it->second;
    }
    // One propagate-mode (mode 1) launch of `mod` - the stepper, or a variant of it - over the device-resident state: every
    // lane runs its own adaptive loop up to its final time or max_steps. scalar_tf: the final time of every lane, or nullptr
    // when the per-lane final times are in d_tfhi / d_tflo already.
    void launch_propagate(device_module &mod, const double *scalar_tf, const std::vector<double> &max_delta_ts,
                          std::size_t max_steps, bool wtc)
    {
        d_counters.zero(stream);
        auto a = base_args();
        if (scalar_tf != nullptr) {
            a.tfin_hi = nullptr;
            a.tfin_lo = nullptr;
            a.tfin_s_hi = *scalar_tf;
            a.tfin_s_lo = 0.;
        }
        if (max_delta_ts.empty()) {
            a.lim = nullptr;
        } else {
            d_lim.upload(max_delta_ts.data(), max_delta_ts.size() * sizeof(double), stream);
            d_lim_src = nullptr;
        }
        if (wtc && is_cluster()) {
            ensure_tc();
            a.tc = d_tc.as<double>();
        }
        a.mode = 1;
        a.max_steps = max_steps;
        keep_written_tc(wtc);
        if (batch_semantics == 0) {
            snapshot_for_rollback();
        }
        mod.launch_taylor(a);
        after_kernel(wtc);
        prop_res_dev_newer = true;
        step_res_dev_newer = false;
    }
    void snapshot_for_rollback()
    {
        const auto sb = d_state.bytes(), tb = d_thi.bytes();
        if (snap_state.bytes() != sb) {
            snap_state = device_buffer(sb, device);
            snap_thi = device_buffer(tb, device);
            snap_tlo = device_buffer(tb, device);
        }
        device_copy(snap_state.get(), d_state.get(), sb, device, stream);
        device_copy(snap_thi.get(), d_thi.get(), tb, device, stream);
        device_copy(snap_tlo.get(), d_tlo.get(), tb, device, stream);
    }
    void rollback_to_snapshot()
    {
        device_copy(d_state.get(), snap_state.get(), d_state.bytes(), device, stream);
        device_copy(d_thi.get(), snap_thi.get(), d_thi.bytes(), device, stream);
        device_copy(d_tlo.get(), snap_tlo.get(), d_tlo.bytes(), device, stream);
        dev_newer = true;
        times_fresh = false;
        host_newer = false;
        // With a host pointer handed out (get_state_data(), hy_tab_set_state(), the Python state setter) the host mirrors
        // are refreshed after every launch and re-uploaded before the next one: they hold the state at the END of the
        // rolled-back propagation, which would overwrite the restored snapshot in the re-run. Bring them back as well.
        refresh_held_mirrors();
    }
    // ---- variational integrators (var_ode_sys.hpp, taylor_map.hpp) ----
    // What a variational integrator knows beyond its (larger) system: immutable, shared by the copies. The module of the
    // Taylor map is compiled with the integrator and loaded at the first evaluation; tstate is the result of the last
    // eval_taylor_map().
    struct var_data {
        var_ode_sys vsys;
        std::string tmap_source;
        std::shared_ptr<const compiled_module> tmap_cmod;
        // Why there is no module (no arguments, or a map beyond what the kernels hold): the message of the evaluations.
        std::string tmap_why;
    };
    std::shared_ptr<const var_data> var;
    mutable std::unique_ptr<aux_module> tmap_mod;
    device_buffer d_tmap_in, d_tmap_out;
    std::vector<double> tstate;
    // Continuous output produced by the last propagate_for/until() with c_output = true.
    std::optional<c_out_core> last_c_out;
    // Post-step kernel of the device-resident propagate_grid() loop (created on first use).
    mutable std::unique_ptr<aux_module> grid_mod;
    // ---- grid observables (grid_observables.hpp) ----
    // The post-step modules with an observable section this integrator has met, keyed by the text of the observables and
    // the way of holding the samples: checked against the system, generated and compiled on first use (the code objects
    // live in the process-wide cache), loaded at the first launch. Nothing is ever dropped: an integrator which meets
    // generated observables without end keeps a section, a source text and a loaded module for each of them. The intended
    // use is a handful of lists per integrator; a copy of the integrator starts with an empty map.
    // (One module per (observables, statistics): with statistics, the module which folds)
    struct go_module : section_module {
        grid_obs_section sec;
    };
    std::map<std::string, go_module> go_modules;
    go_module &get_go_module(const grid_sampling &gs)
    {
        return find_or_build(go_modules, grid_obs_key(gs), "grid observables", [&](go_module &v) {
            v.sec = make_grid_obs_section(gs, state_variables_of(sys), prog.n_par);
            v.source = make_grid_source(order, dim, high_accuracy, &v.sec);
        });
    }

    // ---- event detection (see event_detection.hpp) ----
    std::vector<core_t_event> tes;
    std::vector<core_nt_event> ntes;
    // te_cooldowns[lane][event]: (time elapsed since the trigger, cooldown duration).
    mutable std::vector<std::vector<std::optional<std::pair<double, double>>>> te_cooldowns;
    void *cb_ctx = nullptr;
    mutable std::unique_ptr<aux_module> ed_mod;
    mutable device_buffer d_ev_tc, d_mas, d_geps, d_dirs, d_cd_first, d_cd_second, d_cd_active, d_ed_out, d_ed_counts,
        d_ed_flags, d_ed_wl;
    std::uint64_t ed_slots = 0;
    std::uint64_t ed_failures = 0;
    // Events on the wave-cluster steppers: the main stepper is built from the system alone and runs in mode 4 (jets of
    // the state variables, no update); hy_ev_jets (emit_event_jets(), hip_emit_events.cpp) derives the jets of the event
    // equations and the final step size from them. The companion module ev_emitted / ev_cmod holds it and, on compact
    // coefficients, hy_dout_c and hy_tc_expand - those two alone (emit_compact_tc_module(), dense_output_text.cpp) when the
    // stepper evaluates the event equations itself. tab_core::event_jets_module() shows the module.
    bool cluster_events = false;
    emitted_module ev_emitted;
    std::shared_ptr<const compiled_module> ev_cmod;
    mutable std::unique_ptr<aux_module> evj_mod;
    mutable device_buffer d_selnorms;
    // Set by propagate_for() only: propagate_until() then accepts 2 * N double-length (hi, lo) final times.
    bool dl_times_ok = false;
    // Incremented by set_time() / set_dtime(): lets the device-driven loops detect callbacks that touch the time
    // coordinate without moving the times to the host after every sweep.
    std::uint64_t time_gen = 0;

    [[nodiscard]] bool has_events() const
    {
        return !tes.empty() || !ntes.empty();
    }
    void require_events() const
    {
        if (!has_events()) {
            throw std::invalid_argument("No events were defined for this integrator");
        }
    }
    // (lims == nullptr: the step limits are already in d_lim - device-driven loops. There is no write_tc argument: the
    // Taylor coefficients are always written by the stepper with events, src/taylor_adaptive_batch.cpp:756-757.)
    void step_with_events_device(const std::vector<double> *lims);
    // Its phases, in order (tab_events.cpp); ev_step carries what one phase leaves for the next.
    struct ev_step;
    void ev_launch(ev_step &s, const std::vector<double> *lims);
    void ev_update_state(ev_step &s);
    void ev_apply_on_device(ev_step &s);
    void ev_native_counters(ev_step &s);
    void ev_fetch_records(ev_step &s);
    void ev_host_callbacks(ev_step &s);
    void ev_scatter(ev_step &s);
    void ev_log_host_rows(ev_step &s);
    void ev_final_checks(ev_step &s);
    void ensure_event_buffers();
    void launch_event_stepper(const std::vector<double> *lims);
    void launch_event_detection(bool device_g_eps);
    // Runs f - a pre_hook() or a step callback of fname - which must not move the time coordinate (generation counter).
    template <typename F>
    bool call_keeping_time(const char *fname, const F &f)
    {
        const auto gen = time_gen;
        bool ret = true;
        if constexpr (std::is_void_v<decltype(f())>) {
            f();
        } else {
            ret = f();
        }
        if (time_gen != gen) {
            throw std::runtime_error(std::string("The invocation of the callback passed to ") + fname
                                     + " resulted in the alteration of the time coordinate of the integrator - this is not supported");
        }
        return ret;
    }
    // Terminal-event cooldowns: the device arrays (d_cd_*) are authoritative between steps with events (updated by
    // hy_ev_post / hy_ev_scatter); te_cooldowns is the lazily synchronised host mirror.
    mutable bool cd_dev_newer = false;
    bool cd_host_newer = true;
    // Cooldowns set by the terminal events of the step being processed (position, first, second), not yet on the device:
    // a callback which reads or resets the cooldowns sees them (the reference sets the cooldown before it invokes the
    // callback, src/taylor_adaptive_batch.cpp:875-890).
    mutable std::vector<double> pending_cd;
    void cooldowns_to_host() const;
    void cooldowns_to_device();
    mutable device_buffer d_ev_cursor, d_ev_rec, d_ev_upd, d_ev_counts, d_te_cd;
    // Every event callback is the library's counting callback: hy_ev_post applies the events itself (ep_kargs::native).
    mutable bool ev_native = false;
    // ---- independent semantics (config::batch_semantics == 3) ----
    // Library-side events: counting and recording callbacks; under the independent semantics also the terminal events
    // WITHOUT a callback (plain stops: hy_ev_stop writes the stopping outcome behind hy_ev_native, d_te_stop holds the flags).
    [[nodiscard]] bool event_is_native(const core_t_event &ev) const
    {
        return ev.native_counter != nullptr || ev.recorder || ev.action || (batch_semantics == 3 && !ev.callback);
    }
    // ---- terminal-event actions (core_t_event::action, event_action.hpp) ----
    // One section of the kernel hy_ev_action per terminal event with an action; the module is compiled with the
    // integrator and loaded at the first step which needs it.
    std::vector<event_action_section> act_sections;
    mutable section_module act;
    // Systems [first, first + count): by their outcomes (force < 0) or by the section of the terminal event `force`.
    void launch_event_action(std::uint64_t first, std::uint64_t count, long long force) const
    {
        auto &act_mod = act.loaded(device);
        const eva_kargs ka{d_outcome.as<long long>(), d_state.as<double>(), d_pars.as<double>(), d_thi.as<double>(), N, first, count, force};
        if (ev_timing) {
            // (Event timing on: the duration of the kernel from HIP events, see get_event_action_kernel_ms().)
            act_ms += act_mod.launch_timed("hy_ev_action", count, 256, ka, stream);
            ++act_timed;
        } else {
            act_mod.launch("hy_ev_action", count, 256, ka, stream);
        }
    }
    mutable double act_ms = 0;
    mutable std::uint64_t act_timed = 0;
    // The host-loop path and the marker callback of the C ABI: the action of terminal event te_idx on system i alone,
    // on the newest copy of the state; the mirrors follow as after any kernel.
    void apply_event_action(std::uint32_t te_idx, std::uint32_t i)
    {
        before_kernel();
        launch_event_action(i, 1, static_cast<long long>(te_idx));
        after_kernel(false);
    }
    [[nodiscard]] bool all_events_native() const
    {
        return std::all_of(tes.begin(), tes.end(), [this](const auto &ev) { return event_is_native(ev); })
               && std::all_of(ntes.begin(), ntes.end(), [](const auto &ev) { return ev.native_counter != nullptr || ev.recorder; });
    }
    mutable device_buffer d_te_stop;
    // Sticky outcomes of the systems retired in the running call (0: not retired); the pointer is set while a sweep loop
    // runs, null otherwise. n_retired / n_retired_nf: of the last sweep loop.
    device_buffer d_retired;
    const long long *retired_ptr = nullptr;
    void ensure_grid_mod() const;
    std::uint64_t n_retired = 0, n_retired_nf = 0;
    void log_sweep_loop(const char *what, std::size_t sweeps) const
    {
        if (detail::log_enabled(log_level::debug)) {
            static const char *const names[] = {"reference", "lockstep", "per_lane", "independent"};
            detail::log_message(log_level::debug,
                                std::string(what) + " sweep loop: batch_semantics " + std::to_string(batch_semantics) + " ("
                                    + names[batch_semantics] + "), " + std::to_string(sweeps) + " sweeps, "
                                    + std::to_string(n_retired - n_retired_nf) + " systems retired by events, "
                                    + std::to_string(n_retired_nf) + " retired as non-finite, events applied on the device: "
                                    + ((has_events() && all_events_native()) ? "yes" : "no") + " ("
                                    + std::to_string(act_sections.size()) + " event actions)");
        }
    }
    // What the sweep loops of propagate_until() and propagate_grid() share. Independent semantics (batch_semantics == 3,
    // DESIGN 4.6): a stopping terminal event or a non-finite state retires ONE system (sticky outcome in d_retired, zero-
    // length steps from then on); the loop ends when every system is done or retired.
    struct sweep_ctx {
        impl &d;
        long long *const retired; // d_retired, null unless the semantics are independent
        const bool indep;
        scoped_value<const long long *> guard; // retired_ptr, for the duration of the loop
        // The independent-semantics fields of the argument block of a post-step kernel.
        void fill(grid_kargs &a) const
        {
            a.retired = retired;
            a.outcome_w = indep ? d.d_outcome.as<long long>() : nullptr;
            a.cd_active = (indep && !d.tes.empty()) ? d.d_cd_active.as<int>() : nullptr;
            a.cd_second = (indep && !d.tes.empty()) ? d.d_cd_second.as<double>() : nullptr;
        }
        // Counters of the sweep: the first n_plain, all six (systems retired by events / as non-finite) when independent.
        void read_counters(const device_buffer &b_cnt, unsigned (&cnt)[6], unsigned n_plain) const
        {
            b_cnt.download(cnt, (indep ? 6u : n_plain) * sizeof(unsigned), d.stream);
            d.n_retired = static_cast<std::uint64_t>(cnt[4]) + cnt[5];
            d.n_retired_nf = cnt[5];
        }
        // The loop was ended by the callback or by max_steps: the outcome of the systems neither done nor retired (of all
        // of them with the other semantics, when the results are fetched).
        void override_rest(grid_kargs a, taylor_outcome oc) const
        {
            if (indep) {
                a.override_oc = static_cast<long long>(oc);
                d.grid_mod->launch("hy_indep_override", d.N, 256, a, d.stream);
            } else {
                d.prop_res_override = oc;
            }
        }
    };
    sweep_ctx start_retirement()
    {
        n_retired = 0;
        n_retired_nf = 0;
        n_stopped_by_action = 0;
        long long *r = nullptr;
        if (batch_semantics == 3) {
            if (d_retired.bytes() != N * sizeof(long long)) {
                d_retired = device_buffer(N * sizeof(long long), device);
            }
            d_retired.zero(stream);
            r = d_retired.as<long long>();
        }
        return {*this, r, r != nullptr, {retired_ptr, r}};
    }
    // One sweep - a step of every system, limits as in upload_lims(): the step with events (their callbacks run inside;
    // state, times, outcomes and cooldowns stay on the device) or a plain step.
    void take_sweep_step(const std::vector<double> *lims, bool wtc)
    {
        if (has_events()) {
            step_with_events_device(lims);
        } else {
            run_step(lims, wtc);
        }
    }
    // (Page-locked landing area of the event records of a step: see pinned_buffer.)
    mutable pinned_buffer h_ev_rec;
    // ---- event log (core_*_event::recorder, see event_detection.hpp) ----
    // Rows of log_row_doubles() doubles in d_ev_log, log_rows of them valid; the buffer grows geometrically (device-to-device
    // copy) before the kernels of a step write to it. log_stash: the rows while the integrator moves between devices.
    bool ev_has_rec = false, log_states = true;
    std::shared_ptr<const compiled_module> evr_cmod, drow_cmod;
    mutable std::unique_ptr<aux_module> evr_mod, drow_mod;
    mutable device_buffer d_ev_log, d_evr_isrec, d_evr_lane, d_evr_blk;
    mutable std::uint64_t log_rows = 0, log_reserved = 0;
    mutable std::vector<double> log_stash;
    // ---- event-log observables (event_observables.hpp) ----
    // The list set on the integrator (null: none), its section, the text and the code object of hy_obs_rows: immutable,
    // shared by the copies. The module is loaded on the integrator's device at the first step which fills rows; the staging
    // buffer (staged mode only) holds the samples of the rows of one step and grows with the rows of a step.
    struct log_obs_data {
        std::vector<expression> obs;
        event_obs_section sec;
        std::string source;
        std::shared_ptr<const compiled_module> cm;
    };
    std::shared_ptr<const log_obs_data> log_obs;
    mutable std::unique_ptr<aux_module> obs_mod;
    mutable device_buffer d_obs_stage;
    // The options of the kernels over the rows of the log: those of the stepper, with the layout of ITS coefficients.
    [[nodiscard]] emit_options log_emit_options() const
    {
        auto eo_log = eo;
        eo_log.compact_tc = cluster_events && emitted.compact_tc;
        return eo_log;
    }
    // Whether a kernel fills columns behind the header from the Taylor coefficients of the step.
    [[nodiscard]] bool log_fills() const
    {
        return log_obs || log_states;
    }
    [[nodiscard]] std::uint32_t log_row_doubles() const
    {
        return event_log_header + (log_obs ? log_obs->sec.n_obs : (log_states ? dim : 0u));
    }
    [[nodiscard]] std::uint64_t log_capacity() const
    {
        return d_ev_log.bytes() / (log_row_doubles() * sizeof(double));
    }
    void log_grow(std::uint64_t rows) const
    {
        const auto rb = log_row_doubles() * sizeof(double);
        if (!log_stash.empty()) {
            // (Rows which came from another device.)
            auto st = std::move(log_stash);
            log_stash.clear();
            log_grow(std::max<std::uint64_t>(rows, st.size() * sizeof(double) / rb));
            device_copy(d_ev_log.get(), st.data(), st.size() * sizeof(double), device, stream);
            stream_synchronize(device, stream);
        }
        if (rows <= log_capacity()) {
            return;
        }
        const auto cap = std::max({rows, 2u * log_capacity(), log_reserved, std::uint64_t(1024)});
        device_buffer nb(static_cast<std::size_t>(cap) * rb, device);
        if (d_ev_log.bytes() != 0u) {
            device_copy(nb.get(), d_ev_log.get(), static_cast<std::size_t>(log_rows) * rb, device, stream);
        }
        // (The old buffer is released once the copy has run: the release waits for the device.)
        d_ev_log = std::move(nb);
    }
    void log_fill_states(std::uint64_t first_row, const unsigned long long *d_n_rows, std::uint64_t n_max) const;
    [[nodiscard]] bool is_cluster() const
    {
        // NOTE: true whenever the stepper does not need the tc buffer as its jet scratch (cluster / table
        // kernels, unrolled kernels with register-resident jets): tc is then written only on request.
        return emitted.tc_optional;
    }

    void ensure_tc() const
    {
        if (d_tc.bytes() == 0u) {
            d_tc = device_buffer(static_cast<std::size_t>(dim) * (order + 1u) * N * sizeof(double), device);
            // The Taylor coefficients read as zeros until a step writes them (the reference value-initialises m_tc:
            // test/taylor_adaptive_batch.cpp:741-746 checks it from a step callback).
            d_tc.zero(stream);
        }
    }

    void ensure_device() const
    {
        if (dmod) {
            return;
        }
        dmod = std::make_unique<device_module>(cmod, device);
        dmod->set_stream(stream);
        const auto n = static_cast<std::size_t>(N);
        const auto dsz = sizeof(double);
        d_state = device_buffer(state.size() * dsz, device);
        d_pars = device_buffer(pars.size() * dsz, device);
        d_thi = device_buffer(n * dsz, device);
        d_tlo = device_buffer(n * dsz, device);
        d_lim = device_buffer(n * dsz, device);
        d_tfhi = device_buffer(n * dsz, device);
        d_tflo = device_buffer(n * dsz, device);
        d_lasth = device_buffer(n * dsz, device);
        d_outcome = device_buffer(n * sizeof(long long), device);
        d_minh = device_buffer(n * dsz, device);
        d_maxh = device_buffer(n * dsz, device);
        d_nsteps = device_buffer(n * sizeof(unsigned long long), device);
        if (!is_cluster()) {
            // Unrolled mode: the tc buffer doubles as the jet scratch of the kernel.
            ensure_tc();
        }
        d_counters = device_buffer(16u * sizeof(unsigned), device);
        host_newer = true;
    }

    void to_device() const
    {
        ensure_device();
        if (host_newer) {
            d_state.upload(state.data(), state.size() * sizeof(double), stream);
            d_pars.upload(pars.data(), pars.size() * sizeof(double), stream);
            d_thi.upload(time_hi.data(), time_hi.size() * sizeof(double), stream);
            d_tlo.upload(time_lo.data(), time_lo.size() * sizeof(double), stream);
            host_newer = false;
        }
    }

    void to_host() const
    {
        if (dev_newer) {
            d_state.download(state.data(), state.size() * sizeof(double), stream);
            d_thi.download(time_hi.data(), time_hi.size() * sizeof(double), stream);
            d_tlo.download(time_lo.data(), time_lo.size() * sizeof(double), stream);
            dev_newer = false;
        }
    }

    // (The times alone: 16 B per system where the state is 8 * dim. dev_newer stays set - the state is still pending -
    // and times_fresh remembers that the mirror of the times is current until the next kernel.)
    mutable bool times_fresh = false;
    void times_to_host() const
    {
        if (dev_newer && !times_fresh) {
            d_thi.download(time_hi.data(), time_hi.size() * sizeof(double), stream);
            d_tlo.download(time_lo.data(), time_lo.size() * sizeof(double), stream);
            times_fresh = true;
        }
    }

    // tc_written: the launch was asked to write the Taylor coefficients. The reference's get_tc() holds the coefficients
    // of the last step taken with write_tc (zeros before the first one, src/taylor_adaptive_batch.cpp:756-760): steppers
    // which keep their jets in the tc buffer anyway do not count.
    void after_kernel(bool tc_written = true)
    {
        dev_newer = true;
        times_fresh = false;
        if (tc_written) {
            tc_dev_newer = true;
            // (A launch which stored the coefficients of every lane ends the "mixed steps" state of tc_stale.)
            if (tc_threshold == nullptr) {
                tc_stale = false;
            }
        }
        lasth_dev_newer = true;
        refresh_held_mirrors();
    }
    // (Host mirrors somebody holds a pointer or a reference to: kept current after every launch.)
    void refresh_held_mirrors() const
    {
        if (sticky_host_ptr || sticky_const_refs) {
            to_host();
        } else if (sticky_time_refs) {
            times_to_host();
        }
    }

    // get_tc() holds the coefficients of the last step taken with write_tc (src/taylor_adaptive_batch.cpp:756-760). The
    // steppers which are not wave-cluster kernels use the tc buffer as their jet scratch on EVERY step: before a launch
    // without write_tc overwrites it, a pending (lazily downloaded) set of coefficients is brought to the host mirror.
    void keep_written_tc(bool wtc)
    {
        if (wtc || !tc_dev_newer || is_cluster() || !dmod || d_tc.bytes() == 0u) {
            return;
        }
        const auto sz = static_cast<std::size_t>(dim) * (order + 1u) * N;
        if (tc.size() != sz) {
            tc.assign(sz, 0.);
        }
        d_tc.download(tc.data(), sz * sizeof(double), stream);
        tc_dev_newer = false;
    }

    void before_kernel()
    {
        if (sticky_host_ptr) {
            // The user may have written through a previously-obtained pointer.
            host_newer = true;
        }
        to_device();
    }

    hy_kargs base_args() const
    {
        hy_kargs a{};
        a.state = d_state.as<double>();
        a.pars = d_pars.as<double>();
        a.time_hi = d_thi.as<double>();
        a.time_lo = d_tlo.as<double>();
        a.lim = d_lim.as<double>();
        a.tfin_hi = d_tfhi.as<double>();
        a.tfin_lo = d_tflo.as<double>();
        a.last_h = d_lasth.as<double>();
        a.outcome = d_outcome.as<long long>();
        a.min_h = d_minh.as<double>();
        a.max_h = d_maxh.as<double>();
        a.n_steps = d_nsteps.as<unsigned long long>();
        a.tc = is_cluster() ? nullptr : d_tc.as<double>();
        a.N = N;
        a.max_steps = 0;
        a.mode = 0;
        a.counters = d_counters.as<unsigned>();
        return a;
    }

    // step() / step_backward(): the limits are +-infinity for every lane - kept in two vectors built once, uploaded only
    // when d_lim does not hold them already (8 MB per call for 1 048 576 systems otherwise).
    std::vector<double> lims_pinf, lims_ninf;
    const double *d_lim_src = nullptr;
    const std::vector<double> &inf_lims(bool forward)
    {
        auto &v = forward ? lims_pinf : lims_ninf;
        if (v.size() != N) {
            v.assign(N, forward ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity());
        }
        return v;
    }
    // (lims == nullptr: the step limits are already in d_lim - device-driven loops.)
    void upload_lims(const std::vector<double> *lp)
    {
        if (lp == nullptr) {
            d_lim_src = nullptr;
            return;
        }
        const auto &lims = *lp;
        const bool cached = lims.data() == lims_pinf.data() || lims.data() == lims_ninf.data();
        if (cached && lims.data() == d_lim_src) {
            return;
        }
        d_lim.upload(lims.data(), lims.size() * sizeof(double), stream);
        d_lim_src = cached ? lims.data() : nullptr;
    }

    // (Set by the lock-step loop of propagate_grid(): per-lane times below which a step does not store its Taylor
    // coefficients - emitted_module::tc_by_threshold.)
    const double *tc_threshold = nullptr;
    // One lock-step sweep: a single step for every lane with the per-lane signed limits 'lims' (null: as upload_lims()).
    void run_step(const std::vector<double> *lims, bool wtc)
    {
        before_kernel();
        upload_lims(lims);
        d_counters.zero(stream);
        keep_written_tc(wtc);
        auto a = base_args();
        if (wtc && is_cluster()) {
            ensure_tc();
            a.tc = d_tc.as<double>();
        }
        a.mode = 0;
        if (tc_threshold != nullptr && wtc) {
            a.tfin_hi = tc_threshold;
            a.pad = 4;
        }
        dmod->launch_taylor(a);
        after_kernel(wtc);
        step_res_dev_newer = true;
    }

    void fetch_step_res() const
    {
        if (!step_res_dev_newer) {
            return;
        }
        std::vector<long long> oc(N);
        std::vector<double> h(N);
        d_outcome.download(oc.data(), oc.size() * sizeof(long long), stream);
        d_lasth.download(h.data(), h.size() * sizeof(double), stream);
        for (std::uint32_t i = 0; i < N; ++i) {
            step_res[i] = std::tuple{static_cast<taylor_outcome>(oc[i]), h[i]};
        }
        last_h = h;
        lasth_dev_newer = false;
        step_res_dev_newer = false;
    }

    void fetch_prop_res() const
    {
        if (!prop_res_dev_newer) {
            return;
        }
        std::vector<long long> oc(N);
        std::vector<double> mn(N), mx(N);
        std::vector<unsigned long long> ns(N);
        d_outcome.download(oc.data(), oc.size() * sizeof(long long), stream);
        d_minh.download(mn.data(), mn.size() * sizeof(double), stream);
        d_maxh.download(mx.data(), mx.size() * sizeof(double), stream);
        d_nsteps.download(ns.data(), ns.size() * sizeof(unsigned long long), stream);
        if (fix_step_limit) {
            // The reference stops the whole batch when the iteration counter reaches max_steps and reports step_limit in
            // EVERY lane (src/taylor_adaptive_batch.cpp:1516): the lanes which were done earlier took zero-length steps
            // in the meantime, so their states, times and counters are what the device-resident loop left.
            fix_step_limit = false;
            const auto sl = static_cast<long long>(taylor_outcome::step_limit);
            if (std::find(oc.begin(), oc.end(), sl) != oc.end()) {
                std::fill(oc.begin(), oc.end(), sl);
                d_outcome.upload(oc.data(), oc.size() * sizeof(long long), stream);
            }
        }
        for (std::uint32_t i = 0; i < N; ++i) {
            prop_res[i] = std::tuple{static_cast<taylor_outcome>(oc[i]), mn[i], mx[i], static_cast<std::size_t>(ns[i])};
        }
        prop_res_dev_newer = false;
    }
};

} // namespace heyoka_amd::detail

#endif
