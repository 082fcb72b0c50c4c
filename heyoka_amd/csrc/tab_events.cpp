// Host driver of the MI355X batch Taylor integrator: the step with event detection, the event log, the event actions.
#include "tab_impl.hpp"

namespace heyoka_amd::detail
{

// ---- events ----
bool tab_core::with_events() const
{
    return m_impl->has_events();
}
const std::vector<core_t_event> &tab_core::get_t_events() const
{
    m_impl->require_events();
    return m_impl->tes;
}
const std::vector<core_nt_event> &tab_core::get_nt_events() const
{
    m_impl->require_events();
    return m_impl->ntes;
}
const std::vector<std::vector<std::optional<std::pair<double, double>>>> &tab_core::get_te_cooldowns() const
{
    m_impl->require_events();
    m_impl->cooldowns_to_host();
    return m_impl->te_cooldowns;
}
void tab_core::reset_cooldowns()
{
    for (std::uint32_t i = 0; i < m_impl->N; ++i) {
        reset_cooldowns(i);
    }
}
void tab_core::reset_cooldowns(std::uint32_t i)
{
    m_impl->require_events();
    if (i >= m_impl->N) {
        throw std::invalid_argument("Cannot reset the cooldowns at batch index " + std::to_string(i)
                                    + ": the batch size for this integrator is only " + std::to_string(m_impl->N));
    }
    m_impl->cooldowns_to_host();
    for (auto &cd : m_impl->te_cooldowns[i]) {
        cd.reset();
    }
    m_impl->cd_host_newer = true;
}
void tab_core::set_callback_context(void *ctx)
{
    m_impl->cb_ctx = ctx;
}

// One step with event detection: the event branch of step_impl(), src/taylor_adaptive_batch.cpp:727-1030.
// Device: stepper with events (jets of the state and of the event equations, step size, no state update), event
// detection kernel, dense-output kernel for the state update at the (possibly truncated) step. Host: the
// reference's sequential per-lane logic on the few detected events.
void tab_core::impl::cooldowns_to_host() const
{
    if (!cd_dev_newer) {
        return;
    }
    const auto n = static_cast<std::size_t>(N);
    const auto n_te = tes.size();
    std::vector<double> cf(n_te * n), cs(n_te * n);
    std::vector<int> ca(n_te * n);
    d_cd_first.download(cf.data(), cf.size() * sizeof(double), stream);
    d_cd_second.download(cs.data(), cs.size() * sizeof(double), stream);
    d_cd_active.download(ca.data(), ca.size() * sizeof(int), stream);
    for (std::size_t i = 0; i < n; ++i) {
        for (std::size_t e = 0; e < n_te; ++e) {
            if (ca[e * n + i] != 0) {
                te_cooldowns[i][e].emplace(cf[e * n + i], cs[e * n + i]);
            } else {
                te_cooldowns[i][e].reset();
            }
        }
    }
    for (std::size_t q = 0; q + 2u < pending_cd.size(); q += 3u) {
        const auto pos = static_cast<std::size_t>(pending_cd[q]);
        te_cooldowns[pos % n][pos / n].emplace(pending_cd[q + 1u], pending_cd[q + 2u]);
    }
    cd_dev_newer = false;
}

void tab_core::impl::cooldowns_to_device()
{
    if (!cd_host_newer || tes.empty()) {
        cd_host_newer = false;
        return;
    }
    cooldowns_to_host();
    const auto n = static_cast<std::size_t>(N);
    const auto n_te = tes.size();
    std::vector<double> cf(n_te * n, 0.), cs(n_te * n, 0.);
    std::vector<int> ca(n_te * n, 0);
    for (std::size_t i = 0; i < n; ++i) {
        for (std::size_t e = 0; e < n_te; ++e) {
            if (const auto &cd = te_cooldowns[i][e]) {
                cf[e * n + i] = cd->first;
                cs[e * n + i] = cd->second;
                ca[e * n + i] = 1;
            }
        }
    }
    d_cd_first.upload(cf.data(), cf.size() * sizeof(double), stream);
    d_cd_second.upload(cs.data(), cs.size() * sizeof(double), stream);
    d_cd_active.upload(ca.data(), ca.size() * sizeof(int), stream);
    cd_host_newer = false;
}

void tab_core::impl::ensure_event_buffers()
{
    const auto n = static_cast<std::size_t>(N);
    const auto dsz = sizeof(double);
    const auto n_te = static_cast<std::uint32_t>(tes.size()), n_nte = static_cast<std::uint32_t>(ntes.size());
    const auto n_ev = n_te + n_nte;
    const auto maxd = ed_max_detected(order, n_te, n_nte);
    ensure_tc();
    if (d_ev_tc.bytes() == 0u) {
        // (One spare block: the stepper which takes close-encounter events from the lanes of their pairs lets the lanes
        // WITHOUT an event store there - every statement unconditional.)
        d_ev_tc = device_buffer((static_cast<std::size_t>(n_ev) + 1u) * (order + 1u) * n * dsz, device);
        d_mas = device_buffer(n * dsz, device);
        d_geps = device_buffer(n * dsz, device);
        d_dirs = device_buffer(std::max<std::size_t>(n_ev, 1u) * sizeof(int), device);
        const auto ncd = std::max<std::size_t>(n_te, 1u) * n;
        d_cd_first = device_buffer(ncd * dsz, device);
        d_cd_second = device_buffer(ncd * dsz, device);
        d_cd_active = device_buffer(ncd * sizeof(int), device);
        d_ed_out = device_buffer(2u * n * maxd * 4u * dsz, device);
        d_ed_counts = device_buffer(2u * n * sizeof(unsigned), device);
        d_ed_flags = device_buffer(4u * sizeof(unsigned), device);
        // Working lists of the root isolation: one column per launched thread of hy_detect_events (a grid-stride loop
        // over the lanes). Sized from what the device keeps in flight, not from the ensemble: at least one wavefront per
        // compute unit (64 x 256 columns), at most 1 GiB (42 KB per column at order 20: ~25 000 columns; almost every
        // lane leaves the kernel at the exclusion test and never touches its column) - the previous 4 GiB budget made a
        // large-N integrator with events fail at allocation where nothing needed the space. The lists of detected events
        // (d_ed_out) are 2 * N * (order + 1) * max(n_te, n_nte) * 32 B: 1.4 GB per million systems at order 20, the price
        // of the reference's bound of (order + 1) detections per event and step.
        const auto per_slot = ed_work_list_bytes_per_slot(order);
        const std::uint64_t max_slots = std::clamp<std::uint64_t>((std::uint64_t(1) << 30) / per_slot / 64u * 64u, 64u * 256u, 64u * 256u * 8u);
        ed_slots = std::min<std::uint64_t>((static_cast<std::uint64_t>(n) + 63u) / 64u * 64u, max_slots);
        d_ed_wl = device_buffer(static_cast<std::size_t>(ed_slots) * per_slot, device);
        d_ev_cursor = device_buffer(4u * sizeof(unsigned long long), device);
        // Library-side callbacks only - counting (core_*_event::native_counter) or recording (core_*_event::recorder): the
        // events are applied on the device.
        // (Independent semantics: terminal events without a callback count as library-side, see event_is_native().)
        ev_native = all_events_native();
        std::vector<double> te_cd;
        std::vector<int> is_rec, te_stop;
        for (const auto &ev : tes) {
            te_cd.push_back(ev.cooldown);
            is_rec.push_back(ev.recorder ? 1 : 0);
            te_stop.push_back((batch_semantics == 3 && !ev.callback && !ev.action) ? 1 : 0);
        }
        for (const auto &ev : ntes) {
            is_rec.push_back(ev.recorder ? 1 : 0);
        }
        if (ev_has_rec) {
            drow_mod = std::make_unique<aux_module>(drow_cmod, device);
        }
        if (ev_native && ev_has_rec) {
            evr_mod = std::make_unique<aux_module>(evr_cmod, device);
            d_evr_isrec = device_buffer(is_rec.size() * sizeof(int), device);
            d_evr_isrec.upload(is_rec.data(), is_rec.size() * sizeof(int), stream);
            d_evr_lane = device_buffer(n * sizeof(unsigned), device);
            d_evr_blk = device_buffer(((n + 255u) / 256u) * sizeof(unsigned long long), device);
        }
        if (ev_native) {
            d_ev_counts = device_buffer((tes.size() + ntes.size()) * sizeof(unsigned long long), device);
            d_te_cd = device_buffer(std::max<std::size_t>(te_cd.size(), 1u) * sizeof(double), device);
            if (!te_cd.empty()) {
                d_te_cd.upload(te_cd.data(), te_cd.size() * sizeof(double), stream);
            }
            if (std::any_of(te_stop.begin(), te_stop.end(), [](int f) { return f != 0; })) {
                d_te_stop = device_buffer(te_stop.size() * sizeof(int), device);
                d_te_stop.upload(te_stop.data(), te_stop.size() * sizeof(int), stream);
            }
        }
        std::vector<int> dirs;
        for (const auto &ev : tes) {
            dirs.push_back(static_cast<int>(ev.dir));
        }
        for (const auto &ev : ntes) {
            dirs.push_back(static_cast<int>(ev.dir));
        }
        d_dirs.upload(dirs.data(), dirs.size() * sizeof(int), stream);
        ed_mod = std::make_unique<aux_module>(hiprtc_compile_source(make_event_detection_source(order, maxd)), device);
        cd_host_newer = true;
    }
    if (d_dout.bytes() == 0u) {
        d_dout = device_buffer(d_out.size() * dsz, device);
        d_douth = device_buffer(n * dsz, device);
    }
}

// Stepper with events: jets of the state and of the event equations, step sizes, max |x_i|, no state update.
void tab_core::impl::launch_event_stepper(const std::vector<double> *lims)
{
    const auto n = static_cast<std::size_t>(N);
    const auto dsz = sizeof(double);
    upload_lims(lims);
    d_counters.zero(stream);
    auto a = base_args();
    a.tc = d_tc.as<double>();
    a.ev_tc = d_ev_tc.as<double>();
    a.max_abs_state = d_mas.as<double>();
    a.mode = 4;
    a.pad = 1;
    if (cluster_events && emitted.events_in_stepper) {
        tc_partial = false; // (nobody asked for the coefficients of the previous step: this step replaces them)
        // (The state columns of the event log are evaluated from the coefficients of every lane with a recorded event. The
        // stepper stores them on demand only where a TERMINAL event is possible - where a step may be truncated -, which
        // does not cover the non-terminal events: with recording callbacks and the states on, every step stores them all.)
        const bool all_now = ev_all_tc || tc_regenerated || (ev_has_rec && log_fills());
        tc_regenerated = false;
        if (!all_now) {
            if (evs_state.bytes() == 0u) {
                evs_state = device_buffer(d_state.bytes(), device);
                evs_thi = device_buffer(d_thi.bytes(), device);
                evs_tlo = device_buffer(d_tlo.bytes(), device);
            }
            // (One copy kernel of the event-detection module: see hy_copy_arrays in event_detection.cpp.)
            copy_kargs ca{{evs_state.as<double>(), evs_thi.as<double>(), evs_tlo.as<double>(), nullptr},
                          {d_state.as<double>(), d_thi.as<double>(), d_tlo.as<double>(), nullptr},
                          {d_state.bytes() / dsz, d_thi.bytes() / dsz, d_tlo.bytes() / dsz, 0u}};
            // (Runtime parameters: a callback of this step may change them before somebody asks for the coefficients.)
            if (prog.n_par != 0u && d_pars.bytes() != 0u) {
                if (evs_pars.bytes() != d_pars.bytes()) {
                    evs_pars = device_buffer(d_pars.bytes(), device);
                }
                ca.dst[3] = evs_pars.as<double>();
                ca.src[3] = d_pars.as<double>();
                ca.n[3] = d_pars.bytes() / dsz;
            }
            ed_mod->launch("hy_copy_arrays", std::min<std::uint64_t>(ca.n[0], std::uint64_t(256) * 256u * 16u), 256, ca, stream);
            a.pad = 0;
        }
    }

    if (cluster_events) {
        if (d_selnorms.bytes() == 0u) {
            d_selnorms = device_buffer(3u * n * dsz, device);
            evj_mod = std::make_unique<aux_module>(ev_cmod, device);
        }
        a.sel_norms = d_selnorms.as<double>();
    }
    dmod->launch_taylor(a);
    tc_expand_pending = cluster_events && emitted.compact_tc;
    if (cluster_events && !emitted.events_in_stepper) {
        // Jets of the event equations, extended norms and final step sizes from the jets of the state variables.
        evj_mod->launch("hy_ev_jets", N, 256, a, stream);
    }
}

// Event detection on the device (what failed is counted in d_ed_flags: report_ed_failures()).
void tab_core::impl::launch_event_detection(bool device_g_eps)
{
    const auto n_te = static_cast<std::uint32_t>(tes.size()), n_nte = static_cast<std::uint32_t>(ntes.size());
    d_ed_flags.zero(stream);
    const ed_kargs ea{d_ev_tc.as<double>(),   d_lasth.as<double>(),     d_geps.as<double>(),     d_dirs.as<int>(),
                      d_cd_first.as<double>(), d_cd_second.as<double>(), d_cd_active.as<int>(),   d_ed_out.as<double>(),
                      d_ed_counts.as<unsigned>(), d_ed_flags.as<unsigned>(), N, n_te, n_nte,
                      device_g_eps ? d_mas.as<double>() : nullptr, d_geps.as<double>(), tol,
                      d_ed_wl.as<double>(), ed_slots,
                      // (The stepper which evaluates the event equations itself leaves a flag per system in the buffer of the
                      // selector norms, which it does not use: 0 = no event possible in this step.)
                      (cluster_events && emitted.events_in_stepper) ? d_selnorms.as<double>() : nullptr};
    ed_mod->launch("hy_detect_events", ed_slots, 64, ea, stream);
}

// State columns of n_max rows of the log from first_row on (*d_n_rows of them, if given): dense output of the Taylor
// coefficients of the step at the roots (hy_dout_rows, hip_emit.hpp).
void tab_core::impl::log_fill_states(std::uint64_t first_row, const unsigned long long *d_n_rows, std::uint64_t n_max) const
{
    drow_kargs da{d_ev_log.as<double>() + first_row * log_row_doubles(), d_tc.as<double>(), d_state.as<double>(), d_n_rows,
                  n_max, N, log_row_doubles(), 0u, nullptr, nullptr};
    if (!log_obs) {
        drow_mod->launch("hy_dout_rows", n_max, 256, da, stream);
        return;
    }
    // Event-log observables: hy_obs_rows samples the rows its section reads and stores the observables (event_observables.hpp).
    if (!obs_mod) {
        obs_mod = std::make_unique<aux_module>(log_obs->cm, device);
    }
    da.pars = d_pars.as<double>();
    if (log_obs->sec.staged) {
        // (The samples of the rows of this step, the row index fastest: n_reads * n_max doubles.)
        const auto need = log_obs->sec.reads.size() * static_cast<std::size_t>(n_max) * sizeof(double);
        if (d_obs_stage.bytes() < need) {
            d_obs_stage = device_buffer(std::max(need, 2u * d_obs_stage.bytes()), device);
        }
        da.stage = d_obs_stage.as<double>();
    }
    obs_mod->launch("hy_obs_rows", n_max, 256, da, stream);
}

namespace
{

void report_ed_failures(std::uint64_t &ed_failures, const unsigned (&flags)[3])
{
    const auto total = static_cast<std::uint64_t>(flags[0]) + flags[1] + flags[2];
    if (total != 0u) {
        // The reference logs a warning through its logger and ignores the event for the step when the root isolation
        // exceeds its limits (working list > 250 intervals or more isolating intervals than the order,
        // src/detail/event_detection.cpp:2082-2090) or when the root finder fails (:2150-2165). Here the count is kept
        // (get_event_detection_failures()) and the first occurrence is reported on stderr. The list of detected events
        // of a lane holds (order + 1) entries per event of the class: an overflow cannot come from a successful
        // isolation and is reported separately.
        if (ed_failures == 0u) {
            std::fprintf(stderr,
                         "heyoka_amd: warning: event detection: %u root isolation(s) failed (working list > 250 or more "
                         "isolating intervals than the Taylor order), %u root finding(s) failed, %u event list(s) "
                         "overflowed: the events concerned were ignored in this step\n",
                         flags[0], flags[2], flags[1]);
        }
        ed_failures += total;
    }
}

[[noreturn]] void throw_callback_exceptions(std::vector<std::pair<std::uint32_t, std::exception_ptr>> &cb_eptrs)
{
    if (cb_eptrs.size() == 1u) {
        std::rethrow_exception(cb_eptrs[0].second);
    }
    std::string exc_msg = "Two or more exceptions were raised during the execution of event callbacks in a "
                          "batch integrator:\n\n";
    for (auto &[i, eptr] : cb_eptrs) {
        exc_msg += "Batch index #" + std::to_string(i) + ":\n";
        try {
            std::rethrow_exception(eptr);
        } catch (const std::exception &ex) {
            exc_msg += std::string("    Exception message: ") + ex.what() + "\n";
        } catch (...) {
            exc_msg += "    Exception type: unknown\n    Exception message: unknown\n";
        }
        exc_msg += '\n';
    }
    throw std::runtime_error(exc_msg);
}

} // namespace

// What the phases of one step with events leave for each other, and the timer of the phases.
struct tab_core::impl::ev_step {
    impl &d;
    // Wall-clock time of the phases (tab_core::set_event_timing(), or HEYOKA_AMD_EVENTS_TIMING=1 which also prints them),
    // with a stream synchronisation after each of them.
    const bool to_stderr, timing;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    int lap_idx = 0;
    ev_step(impl &d_, bool env) : d(d_), to_stderr(env), timing(env || d_.ev_timing) {}
    void lap(const char *what)
    {
        if (timing) {
            stream_synchronize(d.device, d.stream);
            const auto now = std::chrono::steady_clock::now();
            const auto ms = std::chrono::duration<double, std::milli>(now - t_last).count();
            if (to_stderr) {
                std::fprintf(stderr, "[events] %-28s %8.3f ms\n", what, ms);
            }
            if (lap_idx < 5) {
                d.ev_ms[lap_idx] += ms;
            }
            ++lap_idx;
            t_last = now;
        }
    }
    ep_kargs pa{};
    // The cursor of the records: [0] doubles needed, [1] written, [2] systems with events, [3] rows of the log.
    unsigned long long cur[4] = {0, 0, 0, 0};
    // Upper bound of the rows the kernels of this step append to the log (0: no recording callback applied on the device).
    std::uint64_t log_ub = 0;
    // Host callbacks: the records of the lanes with events and (lane, offset) of each, in the order of the batch index;
    // what the callback loop leaves - exceptions, outcomes to scatter (the cooldowns are in pending_cd), row headers of the
    // recording callbacks in the order of the log - and the generation of the time coordinate before it ran.
    const double *rec = nullptr;
    struct rec_ref {
        std::uint32_t lane;
        std::size_t off;
    };
    std::vector<rec_ref> refs;
    std::vector<std::pair<std::uint32_t, std::exception_ptr>> cb_eptrs;
    std::vector<double> upd_oc, log_hdrs;
    std::uint64_t gen = 0;
};

// One step with events, per-lane bookkeeping on the device: only the lanes with detected events reach the host (compact
// records), which runs the callbacks and the logic that depends on them (src/taylor_adaptive_batch.cpp:837-1030) in
// the order of the batch index; state, times, step sizes, outcomes and cooldowns stay on the device.
void tab_core::impl::step_with_events_device(const std::vector<double> *lims)
{
    static const bool timing_env = std::getenv("HEYOKA_AMD_EVENTS_TIMING") != nullptr;
    ev_step s(*this, timing_env);
    ev_launch(s, lims);
    ev_update_state(s);
    ev_apply_on_device(s);
    if (ev_native) {
        ev_native_counters(s);
    } else {
        ev_fetch_records(s);
    }
    host_newer = false;
    after_kernel();
    step_res_dev_newer = true;
    cd_dev_newer = !tes.empty();
    if (!ev_native) {
        ev_host_callbacks(s);
        ev_scatter(s);
        ev_log_host_rows(s);
        ev_final_checks(s);
    }
}

// Buffers, stepper, detection, hy_ev_pre (truncation of the steps at the first terminal event, size of the records); the
// flags and the cursor come to the host, the buffers of the records and of the log grow before anything writes to them.
void tab_core::impl::ev_launch(ev_step &s, const std::vector<double> *lims)
{
    const auto dsz = sizeof(double);
    auto &pa = s.pa;
    auto &cur = s.cur;
    ++ev_steps;
    before_kernel();
    ensure_event_buffers();
    cooldowns_to_device();
    s.lap("upload / buffers");

    launch_event_stepper(lims);
    s.lap("stepper (+ event jets)");
    launch_event_detection(true);
    s.lap("detection");

    pa.h = d_lasth.as<double>();
    pa.ed_out = d_ed_out.as<double>();
    pa.counts = d_ed_counts.as<unsigned>();
    pa.dout_h = d_douth.as<double>();
    pa.g_eps = d_geps.as<double>();
    pa.state = d_state.as<double>();
    pa.time_hi = d_thi.as<double>();
    pa.time_lo = d_tlo.as<double>();
    pa.lim = d_lim.as<double>();
    pa.cd_first = d_cd_first.as<double>();
    pa.cd_second = d_cd_second.as<double>();
    pa.cd_active = d_cd_active.as<int>();
    pa.outcome = d_outcome.as<long long>();
    pa.last_h = d_lasth.as<double>();
    pa.cursor = d_ev_cursor.as<unsigned long long>();
    pa.N = N;
    pa.n_te = static_cast<std::uint32_t>(tes.size());
    pa.n_nte = static_cast<std::uint32_t>(ntes.size());
    pa.dim = dim;
    d_ev_cursor.zero(stream);
    ed_mod->launch("hy_ev_pre", N, 256, pa, stream);
    unsigned flags[3] = {0, 0, 0};
    if (ev_native) {
        pa.native = 1;
        pa.ev_counts = d_ev_counts.as<unsigned long long>();
        pa.te_cd = d_te_cd.as<double>();
        d_ev_counts.zero(stream);
    }
    d_ed_flags.download(flags, sizeof(flags), stream);
    if (cluster_events && emitted.events_in_stepper) {
        // (Workgroups of the stepper which did not store their Taylor coefficients: none if it was asked to store all.)
        unsigned cnt[5] = {0, 0, 0, 0, 0};
        d_counters.download(cnt, sizeof(cnt), stream);
        tc_partial = cnt[4] != 0u;
    }
    d_ev_cursor.download(cur, 2u * sizeof(unsigned long long), stream);
    report_ed_failures(ed_failures, flags);
    s.lap("pre + flags to host");
    if (!ev_native && cur[0] * dsz > d_ev_rec.bytes()) {
        d_ev_rec = device_buffer(static_cast<std::size_t>(cur[0] + cur[0] / 2u + 1024u) * dsz, device);
    }
    pa.rec = d_ev_rec.as<double>();
    // Recording callbacks applied on the device: the cursor of hy_ev_pre bounds the rows of this step (4 of its doubles per
    // detected event, 8 more per lane with events); the log grows now, before anything writes to it.
    s.log_ub = (ev_native && ev_has_rec) ? cur[0] / 4u : 0u;
    if (s.log_ub != 0u) {
        log_grow(log_rows + s.log_ub);
    }
}

// State update via dense output at the final step sizes (:781), then hy_ev_post: times / non-finite check / cooldowns /
// outcomes / records.
void tab_core::impl::ev_update_state(ev_step &s)
{
    if (cluster_events && emitted.events_in_stepper) {
        // (The stepper evaluated the event equations, took the final step size and updated the state itself.) Lanes whose
        // step is truncated at a terminal event (dout_h != h) are redone from the Taylor coefficients: their workgroup
        // stored them - a detected event is an event the stepper's exclusion test could not rule out.
        if (!tes.empty()) {
            const doutc_kargs da{d_state.as<double>(), d_tc.as<double>(), d_douth.as<double>(), N, d_lasth.as<double>()};
            evj_mod->launch("hy_dout_c", N, 256, da, stream);
        }
    } else if (tc_expand_pending) {
        // (Compact Taylor coefficients: the dense output derives the rows the stepper left out.)
        const doutc_kargs da{d_state.as<double>(), d_tc.as<double>(), d_douth.as<double>(), N, nullptr};
        evj_mod->launch("hy_dout_c", N, 256, da, stream);
    } else {
        dmod->launch_dout(d_state.as<double>(), d_tc.as<double>(), d_douth.as<double>(), N);
    }
    ed_mod->launch("hy_ev_post", N, 256, s.pa, stream);
}

// Library-side events, applied on the device: counts, cooldowns and outcomes (hy_ev_native), plain stops, rows of the
// log, actions. Nothing to do for host callbacks, or in a step without events.
void tab_core::impl::ev_apply_on_device(ev_step &s)
{
    const auto n_te = s.pa.n_te;
    const bool any = ev_native && s.cur[0] != 0u;
    if (any) {
        ed_mod->launch("hy_ev_native", N, 256, s.pa, stream);
        if (d_te_stop.bytes() != 0u) {
            // Independent semantics: terminal events without a callback are applied on the device as well. hy_ev_native has
            // given them their cooldown and the continuing outcome `index`; hy_ev_stop (post-step module: the text of the
            // event-detection module is pinned) turns it into the stopping outcome -index - 1 where the flag is set.
            const ev_stop_kargs sa{d_outcome.as<long long>(), d_te_stop.as<int>(), N, n_te, 0u};
            ensure_grid_mod();
            grid_mod->launch("hy_ev_stop", N, 256, sa, stream);
        }
    }
    if (s.log_ub != 0u) {
        // Rows of the log from the events of this step (event_detection.hpp): rows per lane and per workgroup, exclusive
        // scan of the workgroup sums (the total lands in the spare word of the cursor, which the host reads anyway), row
        // headers in batch order, state columns by dense output over the rows.
        evr_kargs ra{};
        ra.ed_out = d_ed_out.as<double>();
        ra.counts = d_ed_counts.as<unsigned>();
        ra.dout_h = d_douth.as<double>();
        ra.time_hi = d_thi.as<double>();
        ra.time_lo = d_tlo.as<double>();
        ra.outcome = d_outcome.as<long long>();
        ra.is_rec = d_evr_isrec.as<int>();
        ra.lane_rows = d_evr_lane.as<unsigned>();
        ra.blk = d_evr_blk.as<unsigned long long>();
        ra.total = d_ev_cursor.as<unsigned long long>() + 3;
        ra.rows = d_ev_log.as<double>() + log_rows * log_row_doubles();
        ra.N = N;
        ra.n_te = n_te;
        ra.n_nte = s.pa.n_nte;
        ra.row_doubles = log_row_doubles();
        evr_mod->launch("hy_evr_count", N, 256, ra, stream);
        evr_mod->launch("hy_evr_scan", 256, 256, ra, stream);
        evr_mod->launch("hy_evr_write", N, 256, ra, stream);
        if (log_fills()) {
            log_fill_states(log_rows, ra.total, s.log_ub);
        }
    }
    if (any && act.cm) {
        // Terminal-event actions: hy_ev_native has given the first terminal event of a system its cooldown and the
        // continuing outcome `index`; the rows of the log (a terminal row copies the state) are written. One lane per
        // system, the systems without such an outcome leave after one load.
        launch_event_action(0, N, -1);
    }
}

// The events were applied by hy_ev_post (counts per event, cooldown and outcome of the first terminal event of a lane):
// what is left of the host loop of src/taylor_adaptive_batch.cpp:837-1030 is adding the counts to the callbacks' counters
// - no records, no per-event work. (The reference runs the callbacks one by one in batch order; a counter does not see
// the order.)
void tab_core::impl::ev_native_counters(ev_step &s)
{
    auto &cur = s.cur;
    std::vector<unsigned long long> cnts(tes.size() + ntes.size(), 0u);
    if (cur[0] != 0u) {
        d_ev_counts.download(cnts.data(), cnts.size() * sizeof(unsigned long long), stream);
        d_ev_cursor.download(cur, sizeof(cur), stream);
        ev_systems += cur[2];
        if (s.log_ub != 0u) {
            log_rows += cur[3];
        }
    } else {
        stream_synchronize(device, stream);
    }
    for (std::size_t e = 0; e < cnts.size(); ++e) {
        auto *ctr = e < tes.size() ? tes[e].native_counter : ntes[e - tes.size()].native_counter;
        // (A recording callback may come without a counter.)
        if (ctr != nullptr) {
            __atomic_fetch_add(ctr, static_cast<std::uint64_t>(cnts[e]), __ATOMIC_RELAXED);
        }
    }
    s.lap("dout + post + records");
}

// Host callbacks: the records of the lanes with events, and their order.
void tab_core::impl::ev_fetch_records(ev_step &s)
{
    const auto dsz = sizeof(double);
    auto &cur = s.cur;
    std::size_t rec_size = 0;
    if (cur[0] != 0u) {
        d_ev_cursor.download(cur, 2u * sizeof(unsigned long long), stream);
        rec_size = static_cast<std::size_t>(cur[1]);
        if (cur[1] != 0u) {
            auto *dst = static_cast<double *>(h_ev_rec.reserve(rec_size * dsz));
            d_ev_rec.download(dst, rec_size * dsz, stream);
            s.rec = dst;
        }
    } else {
        stream_synchronize(device, stream);
    }
    s.lap("dout + post + records");
    // Records in the order of the batch index (the compaction kernel appends them in the order its lanes get there): an
    // index of (lane, offset) pairs, sorted.
    for (std::size_t p = 0; p < rec_size;) {
        const auto *r = s.rec + p;
        s.refs.push_back({static_cast<std::uint32_t>(r[0]), p});
        p += 8u + 4u * (static_cast<std::size_t>(r[1]) + static_cast<std::size_t>(r[2]));
        ++ev_systems;
    }
    std::sort(s.refs.begin(), s.refs.end(), [](const auto &x, const auto &y) { return x.lane < y.lane; });
}

// The reference's sequential per-lane logic on the detected events (src/taylor_adaptive_batch.cpp:837-1030).
void tab_core::impl::ev_host_callbacks(ev_step &s)
{
    const auto n = static_cast<std::size_t>(N);
    const auto *const rec = s.rec;
    auto &cb_eptrs = s.cb_eptrs;
    auto &upd_oc = s.upd_oc;
    // The events of a record are unpacked into two scratch lists which are reused from record to record - with 10^5
    // systems reporting events per step a pair of heap-allocated lists per record was most of the host time of a step.
    struct lane_rec {
        std::uint32_t lane = 0;
        double g_eps = 0, h = 0, thi = 0, tlo = 0;
        std::vector<detected_event> tes, ntes;
    } lr;

    auto &upd_cd = pending_cd;
    upd_cd.clear();
    s.gen = time_gen;
    // Row headers of the recording callbacks among the host callbacks: collected where the callback runs, i.e. in the
    // order of the log.
    const auto log_header = [&](std::uint32_t lane, int cls, const detected_event &ev, const dfloat &new_time, double h) {
        const auto tt = new_time - h + ev.root;
        s.log_hdrs.insert(s.log_hdrs.end(), {static_cast<double>(lane), static_cast<double>(cls), static_cast<double>(ev.idx),
                                             static_cast<double>(ev.d_sgn), tt.hi, tt.lo, ev.root, ev.abs_der});
    };
    for (const auto &ref : s.refs) {
        {
            const auto *r = rec + ref.off;
            lr.lane = ref.lane;
            lr.g_eps = r[3];
            lr.h = r[4];
            lr.thi = r[5];
            lr.tlo = r[6];
            lr.tes.clear();
            lr.ntes.clear();
            const auto c_te = static_cast<unsigned>(r[1]), c_nte = static_cast<unsigned>(r[2]);
            const auto *e = r + 8;
            for (unsigned c = 0; c < c_te + c_nte; ++c, e += 4) {
                (c < c_te ? lr.tes : lr.ntes).push_back({static_cast<std::uint32_t>(e[0]), e[1], static_cast<int>(e[2]), e[3]});
            }
        }
        // (Stable, by |root|: src/detail/event_detection.cpp:771-781. Insertion sort: the lists hold one or two events and
        // std::stable_sort() asks the allocator for a buffer every time.)
        const auto sort_by_root = [](std::vector<detected_event> &v) {
            for (std::size_t a_ = 1; a_ < v.size(); ++a_) {
                const auto x = v[a_];
                auto b_ = a_;
                for (; b_ > 0u && std::abs(x.root) < std::abs(v[b_ - 1u].root); --b_) {
                    v[b_] = v[b_ - 1u];
                }
                v[b_] = x;
            }
        };
        sort_by_root(lr.tes);
        sort_by_root(lr.ntes);
        const auto i = lr.lane;
        const auto h = lr.h;
        const auto new_time = dfloat(lr.thi, lr.tlo);

        // Non-terminal events triggering before the first terminal event (:837-871).
        bool nt_cb_exception = false;
        for (const auto &ev : lr.ntes) {
            if (!lr.tes.empty() && !(std::abs(ev.root) < std::abs(h))) {
                break;
            }
            try {
                ntes[ev.idx].callback(cb_ctx, static_cast<double>(new_time - h + ev.root), ev.d_sgn, i);
            } catch (...) {
                cb_eptrs.emplace_back(i, std::current_exception());
                nt_cb_exception = true;
                break;
            }
            if (ntes[ev.idx].recorder) {
                log_header(i, 1, ev, new_time, h);
            }
        }
        if (nt_cb_exception || lr.tes.empty()) {
            continue;
        }

        // The first terminal event (:875-908).
        const auto &ev = lr.tes[0];
        auto &te = tes[ev.idx];
        auto cd = te.cooldown;
        if (!(cd >= 0)) {
            // taylor_deduce_cooldown(), src/detail/event_detection.cpp:519-550.
            cd = lr.g_eps / ev.abs_der * 10;
            if (!std::isfinite(cd)) {
                cd = 0;
            }
        }
        upd_cd.insert(upd_cd.end(), {static_cast<double>(static_cast<std::size_t>(ev.idx) * n + i), 0., cd});
        if (!cd_dev_newer) {
            // (An earlier callback of this step moved the cooldowns to the host: the mirror is the authoritative copy.)
            te_cooldowns[i][ev.idx].emplace(0., cd);
        }
        bool te_cb_ret = false;
        if (te.action) {
            // (The same compiled section as on the device path, restricted to this system: the callbacks which run later
            // in the step see the changed state.)
            try {
                apply_event_action(ev.idx, i);
                te_cb_ret = true;
            } catch (...) {
                cb_eptrs.emplace_back(i, std::current_exception());
                continue;
            }
        } else if (te.callback) {
            try {
                te_cb_ret = te.callback(cb_ctx, ev.d_sgn, i);
            } catch (...) {
                cb_eptrs.emplace_back(i, std::current_exception());
                continue;
            }
        }
        if (te.recorder) {
            log_header(i, 0, ev, new_time, h);
        }
        const auto ev_idx = static_cast<std::int64_t>(ev.idx);
        upd_oc.insert(upd_oc.end(), {static_cast<double>(i), static_cast<double>(te_cb_ret ? ev_idx : (-ev_idx - 1))});
    }
}

// Cooldowns and outcomes set by the callback loop: to the device arrays (hy_ev_scatter).
void tab_core::impl::ev_scatter(ev_step &s)
{
    const auto dsz = sizeof(double);
    auto &pa = s.pa;
    const auto &upd_cd = pending_cd;
    if (!upd_cd.empty() || !s.upd_oc.empty()) {
        // NOTE: a callback may have moved the host mirrors ahead (mutable getters): the device arrays touched here
        // (cooldowns, outcomes) are not among those it can reach.
        std::vector<double> upd(upd_cd);
        upd.insert(upd.end(), s.upd_oc.begin(), s.upd_oc.end());
        if (upd.size() * dsz > d_ev_upd.bytes()) {
            d_ev_upd = device_buffer((upd.size() * 2u + 64u) * dsz, device);
        }
        d_ev_upd.upload(upd.data(), upd.size() * dsz, stream);
        pa.upd = d_ev_upd.as<double>();
        pa.n_cd = static_cast<unsigned>(upd_cd.size() / 3u);
        pa.n_oc = static_cast<unsigned>(s.upd_oc.size() / 2u);
        ed_mod->launch("hy_ev_scatter", pa.n_cd + pa.n_oc, 256, pa, stream);
        stream_synchronize(device, stream);
    }
    pending_cd.clear();
}

// Rows of the recording callbacks which ran on the host. Behind the existing rows: the headers (state columns zeroed),
// then the dense-output kernel of the device path.
void tab_core::impl::ev_log_host_rows(ev_step &s)
{
    const auto &log_hdrs = s.log_hdrs;
    if (log_hdrs.empty()) {
        return;
    }
    const auto w = log_row_doubles();
    const std::uint64_t n_new = log_hdrs.size() / event_log_header;
    log_grow(log_rows + n_new);
    std::vector<double> rows_h(static_cast<std::size_t>(n_new) * w, 0.);
    for (std::uint64_t r = 0; r < n_new; ++r) {
        std::copy_n(log_hdrs.data() + r * event_log_header, event_log_header, rows_h.data() + r * w);
    }
    device_copy(d_ev_log.as<double>() + log_rows * w, rows_h.data(), rows_h.size() * sizeof(double), device, stream);
    if (log_fills()) {
        log_fill_states(log_rows, nullptr, n_new);
    }
    stream_synchronize(device, stream);
    log_rows += n_new;
}

// The exceptions of the callbacks, and a callback which moved the time coordinate.
void tab_core::impl::ev_final_checks(ev_step &s)
{
    const auto n = static_cast<std::size_t>(N);
    if (!s.cb_eptrs.empty()) {
        throw_callback_exceptions(s.cb_eptrs);
    }
    if (time_gen != s.gen) {
        // A callback went through set_time() / set_dtime(): compare the host mirror with the times of the device.
        std::vector<double> thi(n), tlo(n);
        d_thi.download(thi.data(), n * sizeof(double), stream);
        d_tlo.download(tlo.data(), n * sizeof(double), stream);
        for (std::uint32_t i = 0; i < N; ++i) {
            const auto same = [](double x, double y) { return x == y || (std::isnan(x) && std::isnan(y)); };
            if (!same(time_hi[i], thi[i]) || !same(time_lo[i], tlo[i])) {
                throw std::runtime_error("The invocation of one or more event callbacks resulted in the alteration of the "
                                         "time coordinate of the integrator at the batch index "
                                         + std::to_string(i) + " - this is not supported");
            }
        }
    }
}

// ---- event log ----
std::uint64_t tab_core::get_event_log_size() const
{
    return m_impl->log_rows;
}

std::uint32_t tab_core::get_event_log_row_size() const
{
    return m_impl->log_row_doubles();
}

std::uint64_t tab_core::get_event_log_capacity() const
{
    return m_impl->log_capacity();
}

void tab_core::get_event_log(std::uint64_t first, std::uint64_t count, double *out) const
{
    const auto &d = *m_impl;
    if (first > d.log_rows || count > d.log_rows - first) {
        throw std::out_of_range("Invalid range of rows requested from the event log: [" + std::to_string(first) + ", "
                                + std::to_string(first) + " + " + std::to_string(count) + ") of " + std::to_string(d.log_rows));
    }
    if (count == 0u) {
        return;
    }
    const auto w = d.log_row_doubles();
    if (!d.log_stash.empty()) {
        std::copy_n(d.log_stash.data() + first * w, count * w, out);
        return;
    }
    device_copy(out, d.d_ev_log.as<double>() + first * w, static_cast<std::size_t>(count) * w * sizeof(double), d.device, d.stream);
    stream_synchronize(d.device, d.stream);
}

std::vector<double> tab_core::get_event_log() const
{
    std::vector<double> ret(static_cast<std::size_t>(m_impl->log_rows) * m_impl->log_row_doubles());
    get_event_log(0, m_impl->log_rows, ret.data());
    return ret;
}

const double *tab_core::event_log_device() const
{
    const auto &d = *m_impl;
    if (d.log_rows == 0u) {
        return nullptr;
    }
    d.log_grow(d.log_rows);
    stream_synchronize(d.device, d.stream);
    return d.d_ev_log.as<double>();
}

void tab_core::clear_event_log()
{
    m_impl->log_rows = 0;
    m_impl->log_stash.clear();
}

void tab_core::event_log_reserve(std::uint64_t rows)
{
    auto &d = *m_impl;
    d.log_reserved = std::max(d.log_reserved, rows);
    // (Nothing is allocated before the device is in use, nor for an integrator without recording callbacks.)
    if (d.ev_has_rec && d.dmod) {
        d.log_grow(rows);
    }
}

void tab_core::set_event_log_states(bool on)
{
    auto &d = *m_impl;
    if (on == d.log_states) {
        return;
    }
    // (While observables are set the switch does not shape the rows: it is free to move, and the list can be cleared only on an
    // empty log anyway.)
    if (d.log_rows != 0u && !d.log_obs) {
        throw std::invalid_argument("The state columns of the event log can be switched only while the log is empty: it holds "
                                    + std::to_string(d.log_rows) + " row(s) - clear it first");
    }
    d.log_states = on;
}

bool tab_core::get_event_log_states() const
{
    return m_impl->log_states;
}

bool tab_core::has_event_recorders() const
{
    return m_impl->ev_has_rec;
}

const std::vector<char> &tab_core::event_log_code_object(int which) const
{
    const auto &d = *m_impl;
    if (which == 2 && d.ev_has_rec) {
        if (!d.log_obs) {
            throw std::invalid_argument("This integrator has no event-log observables: no observable kernel was compiled");
        }
        return d.log_obs->cm->code;
    }
    const auto &m = which == 0 ? d.evr_cmod : d.drow_cmod;
    if (!m) {
        throw std::invalid_argument("This integrator has no recording event callbacks: no event-log kernels were compiled");
    }
    return m->code;
}

void tab_core::set_event_log_observables(std::optional<std::vector<expression>> obs)
{
    auto &d = *m_impl;
    if (!d.ev_has_rec) {
        throw std::invalid_argument("This integrator has no recording event callbacks: there is no event log to put observables into");
    }
    if (!obs && !d.log_obs) {
        return;
    }
    if (d.log_rows != 0u) {
        throw std::invalid_argument("The observables of the event log can be set or cleared only while the log is empty: it holds "
                                    + std::to_string(d.log_rows) + " row(s) - clear it first");
    }
    if (!obs) {
        d.log_obs.reset();
        d.obs_mod.reset();
        return;
    }
    // (The code object lives in the process-wide cache, keyed by the text: the observables and the options of the emitter.)
    auto v = std::make_shared<impl::log_obs_data>();
    v->sec = make_event_obs_section(*obs, state_variables_of(d.sys), d.prog.n_par);
    v->source = make_event_log_obs_source(d.prog, d.log_emit_options(), v->sec);
    const stopwatch sw;
    v->cm = hiprtc_compile_source(v->source);
    log_message(log_level::trace, "event-log observables: kernel compilation runtime: " + sw.str());
    v->obs = std::move(*obs);
    d.log_obs = std::move(v);
    d.obs_mod.reset();
}

const std::vector<expression> *tab_core::get_event_log_observables() const
{
    return m_impl->log_obs ? &m_impl->log_obs->obs : nullptr;
}

std::string tab_core::event_log_source(int which) const
{
    const auto &d = *m_impl;
    if (!d.ev_has_rec) {
        throw std::invalid_argument("This integrator has no recording event callbacks: no event-log kernels were compiled");
    }
    if (which == 2) {
        if (!d.log_obs) {
            throw std::invalid_argument("This integrator has no event-log observables: no observable kernel was compiled");
        }
        return d.log_obs->source;
    }
    if (which != 1) {
        throw std::invalid_argument("The event-log kernels with a source text of their own are 1 (hy_dout_rows) and 2 (hy_obs_rows)");
    }
    return make_event_log_dout_source(d.prog, d.log_emit_options());
}

std::uint32_t tab_core::get_n_event_actions() const
{
    return static_cast<std::uint32_t>(m_impl->act_sections.size());
}

std::pair<double, std::uint64_t> tab_core::get_event_action_kernel_ms() const
{
    return {m_impl->act_ms, m_impl->act_timed};
}

tab_core::module_view tab_core::event_action_module() const
{
    if (!m_impl->act.cm) {
        throw std::invalid_argument("This integrator has no event actions: no action kernel was compiled");
    }
    return {m_impl->act.source, m_impl->act.cm->code};
}

tab_core::module_view tab_core::event_jets_module() const
{
    if (!m_impl->ev_cmod) {
        throw std::invalid_argument("This integrator has no companion module of a wave-cluster stepper with events: no such "
                                    "kernel was compiled");
    }
    return {m_impl->ev_emitted.source, m_impl->ev_cmod->code};
}

void tab_core::apply_event_action(const event_action &act, std::uint32_t batch_idx)
{
    auto &d = *m_impl;
    if (batch_idx >= d.N) {
        throw std::invalid_argument("Invalid batch index " + std::to_string(batch_idx) + " passed to an event action: the batch size is "
                                    + std::to_string(d.N));
    }
    for (std::size_t e = 0; e < d.tes.size(); ++e) {
        if (d.tes[e].action && d.tes[e].action->assignments == act.assignments) {
            d.apply_event_action(static_cast<std::uint32_t>(e), batch_idx);
            stream_synchronize(d.device, d.stream);
            return;
        }
    }
    throw std::invalid_argument("The event action " + act.to_string() + " does not belong to a terminal event of this integrator");
}

void tab_core::set_event_timing(bool on)
{
    m_impl->ev_timing = on;
}

std::array<double, 8> tab_core::get_event_stats() const
{
    const auto &d = *m_impl;
    return {static_cast<double>(d.ev_steps), d.ev_ms[0], d.ev_ms[1], d.ev_ms[2], d.ev_ms[3], d.ev_ms[4],
            static_cast<double>(d.tc_regens), static_cast<double>(d.ev_systems)};
}

std::uint64_t tab_core::get_n_retired() const
{
    return m_impl->n_retired;
}

bool tab_core::events_on_device() const
{
    return m_impl->has_events() && m_impl->all_events_native();
}

} // namespace heyoka_amd::detail
