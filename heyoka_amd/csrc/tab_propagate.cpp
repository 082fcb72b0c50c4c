// Host driver of the MI355X batch Taylor integrator: step(), propagate_for / _until / _grid() and their sweep loops.
#include "tab_impl.hpp"

namespace heyoka_amd::detail
{

namespace
{

// The max_delta_ts argument of fname: empty or one per system, neither nan nor non-positive.
void check_max_delta_ts(const std::vector<double> &max_delta_ts, std::uint32_t N, const std::string &fname)
{
    if (!max_delta_ts.empty() && max_delta_ts.size() != N) {
        throw std::invalid_argument("Invalid number of max timesteps specified in a Taylor integrator in batch mode: "
                                    "the batch size is "
                                    + std::to_string(N) + ", but the number of specified timesteps is "
                                    + std::to_string(max_delta_ts.size()));
    }
    for (const auto dt : max_delta_ts) {
        if (std::isnan(dt)) {
            throw std::invalid_argument("A nan max_delta_t was passed to the " + fname
                                        + " function of an adaptive Taylor integrator in batch mode");
        }
        if (dt <= 0) {
            throw std::invalid_argument("A non-positive max_delta_t was passed to the " + fname
                                        + " function of an adaptive Taylor integrator in batch mode");
        }
    }
}

// Limit of the first step of a sweep loop: the remaining time, clamped to max_delta_t in the direction of the propagation.
double first_step_limit(const dfloat &rem, int t_dir, double mdt)
{
    return static_cast<double>(t_dir != 0 ? std::min(dfloat(mdt), rem) : std::max(dfloat(-mdt), rem));
}

// The records of a call with ensemble statistics and / or histograms to the caller: raw holds the ens_words words of the
// former, then the counters of the latter. retval, if not null, receives the values of the ensemble statistics followed by the
// counters as doubles; grid_call::ens_raw and hist_raw receive the words of their region.
void give_records(const grid_obs_section &sec, const tab_core::grid_call &call, std::vector<std::uint64_t> raw, std::size_t ens_words,
                  std::vector<double> *retval)
{
    if (retval != nullptr) {
        std::size_t n_vals = 0;
        if (ens_words != 0u) {
            const auto n_rec = ens_words / sec.ens_rec.words;
            ens_finish(sec.ens_rec, sec.ens, raw.data(), n_rec, retval->data());
            n_vals = n_rec * sec.ens.size();
        }
        for (std::size_t w = ens_words; w < raw.size(); ++w) {
            (*retval)[n_vals + (w - ens_words)] = static_cast<double>(raw[w]);
        }
    }
    if (call.hist_raw != nullptr) {
        call.hist_raw->assign(raw.begin() + static_cast<std::ptrdiff_t>(ens_words), raw.end());
    }
    if (call.ens_raw != nullptr) {
        raw.resize(ens_words);
        *call.ens_raw = std::move(raw);
    }
}

} // namespace

// ---- stepping (reference: src/taylor_adaptive_batch.cpp:1039-1080) ----
void tab_core::step(bool wtc)
{
    m_impl->take_sweep_step(&m_impl->inf_lims(true), wtc);
}

void tab_core::step_backward(bool wtc)
{
    m_impl->take_sweep_step(&m_impl->inf_lims(false), wtc);
}

void tab_core::step(const std::vector<double> &max_delta_ts, bool wtc)
{
    auto &d = *m_impl;
    if (max_delta_ts.size() != d.N) {
        throw std::invalid_argument("Invalid number of max timesteps specified in a Taylor integrator in batch mode: "
                                    "the batch size is "
                                    + std::to_string(d.N) + ", but the number of specified timesteps is "
                                    + std::to_string(max_delta_ts.size()));
    }
    if (std::any_of(max_delta_ts.begin(), max_delta_ts.end(), [](double x) { return std::isnan(x); })) {
        throw std::invalid_argument("Cannot invoke the step() function of an adaptive Taylor integrator in batch "
                                    "mode if one of the max timesteps is nan");
    }
    d.take_sweep_step(&max_delta_ts, wtc);
}

// Reference: propagate_for_impl(), src/taylor_adaptive_batch.cpp:1082-1118.
// Reference outcomes on the device-resident propagation (config::batch_semantics == 0, the default). In the reference
// every iteration of propagate_until() steps ALL the lanes of the batch; a lane which produces a non-finite state stops
// the whole batch at that iteration (src/taylor_adaptive_batch.cpp:1404-1407, :1462-1467) and max_steps counts iterations of
// the batch (:1516). The device-resident loop runs every lane on its own. Its results are the reference's whenever no lane
// goes non-finite (finished lanes take zero-length steps in the reference: nothing changes) up to the outcome of a
// step-limited batch, which is fixed when the results are fetched (impl::fetch_prop_res()). A batch WITH a non-finite
// lane - an error path - is rolled back to the snapshot taken before the launch and re-run through the lock-step loop,
// which implements the reference's semantics iteration by iteration.
void tab_core::finish_device_propagate(const std::vector<double> &ts, std::size_t max_steps,
                                       const std::vector<double> &max_delta_ts, bool wtc, const cb_t &cb)
{
    auto &d = *m_impl;
    if (d.batch_semantics != 0) {
        return;
    }
    d.fix_step_limit = max_steps != 0u;
    unsigned nf = 0;
    // (One 4-byte download per call: it waits for the launch, i.e. propagate_*() is synchronous in this mode;
    // batch_semantics = 2 keeps the fully asynchronous per-lane behaviour.)
    d.d_counters.download(&nf, sizeof(unsigned), d.stream);
    if (nf == 0u) {
        return;
    }
    d.fix_step_limit = false;
    d.rollback_to_snapshot();
    const scoped_value<bool> guard(d.force_lockstep, true);
    // (cb: the fused angle reduction falls back to the callback after every sweep; its pre_hook() has run already.)
    propagate_until(ts, max_steps, max_delta_ts, {.call = cb}, wtc, false);
}

void tab_core::propagate_for(const std::vector<double> &delta_ts, std::size_t max_steps,
                             const std::vector<double> &max_delta_ts, const step_hooks &hooks, bool wtc, bool c_out)
{
    auto &d = *m_impl;
    if (delta_ts.size() != 1u && delta_ts.size() != d.N) {
        throw std::invalid_argument("Invalid number of time intervals specified in a Taylor integrator in batch "
                                    "mode: the batch size is "
                                    + std::to_string(d.N) + ", but the number of specified time intervals is "
                                    + std::to_string(delta_ts.size()));
    }
    d.times_to_host();
    std::vector<double> ts(2u * static_cast<std::size_t>(d.N));
    for (std::uint32_t i = 0; i < d.N; ++i) {
        const auto dt = delta_ts.size() == 1u ? delta_ts[0] : delta_ts[i];
        const auto tf = dfloat(d.time_hi[i], d.time_lo[i]) + dt;
        ts[i] = tf.hi;
        ts[d.N + i] = tf.lo;
    }
    // NOTE: double-length final times travel as a vector of size 2 * N: a form accepted only from here (a public
    // propagate_until() call with any size other than N throws like the reference).
    const scoped_value<bool> guard(d.dl_times_ok, true);
    propagate_until(ts, max_steps, max_delta_ts, hooks, wtc, c_out);
}

// Reference: propagate_until_impl(), src/taylor_adaptive_batch.cpp:1137-1534.
void tab_core::propagate_until(const std::vector<double> &ts_, std::size_t max_steps,
                               const std::vector<double> &max_delta_ts, const step_hooks &hooks, bool wtc, bool c_out)
{
    const auto &[cb, pre, red, lib_cb] = hooks;
    auto &d = *m_impl;
    const auto N = d.N;
    d.cb_is_library = cb && lib_cb;
    d.n_retired = 0;
    d.n_retired_nf = 0;
    d.n_stopped_by_action = 0;
    // (The re-run of a rolled-back fused propagation keeps the kind of its callback.)
    if (!d.force_lockstep) {
        d.cb_is_reducer = cb && red;
    }
    d.last_cb_path = 0;

    // Fast path: state and time live on the device (they were produced by a previous kernel), scalar final
    // time, no callback -> nothing to move or to inspect on the host. The per-lane checks of the reference on
    // the *current* times are subsumed by the kernel: a lane whose time is already non-finite (it can only
    // come from an earlier err_nf_state) reports err_nf_state again instead of raising an exception.
    d.last_c_out.reset();
    if (!cb && !c_out && !d.has_events() && ts_.size() == 1u && d.dev_newer && !d.host_newer && !d.sticky_host_ptr
        && d.dmod && d.batch_semantics != 1 && !d.force_lockstep) {
        if (!std::isfinite(ts_[0])) {
            throw std::invalid_argument("A non-finite time was passed to the propagate_until() function of an "
                                        "adaptive Taylor integrator in batch mode");
        }
        check_max_delta_ts(max_delta_ts, N, "propagate_until()");
        d.prop_res_override.reset();
        d.fix_step_limit = false;
        d.launch_propagate(*d.dmod, &ts_[0], max_delta_ts, max_steps, wtc);
        finish_device_propagate(ts_, max_steps, max_delta_ts, wtc);
        return;
    }

    std::vector<double> tf_hi(N), tf_lo(N, 0.);
    if (ts_.size() == 1u) {
        std::fill(tf_hi.begin(), tf_hi.end(), ts_[0]);
    } else if (ts_.size() == N) {
        tf_hi = ts_;
    } else if (d.dl_times_ok && ts_.size() == 2u * static_cast<std::size_t>(N)) {
        std::copy(ts_.begin(), ts_.begin() + N, tf_hi.begin());
        std::copy(ts_.begin() + N, ts_.end(), tf_lo.begin());
    } else {
        throw std::invalid_argument("Invalid number of time limits specified in a Taylor integrator in batch mode: "
                                    "the batch size is "
                                    + std::to_string(N) + ", but the number of specified time limits is "
                                    + std::to_string(ts_.size()));
    }

    d.times_to_host();
    const auto nonfinite = [](double t) { return !std::isfinite(t); };
    if (std::any_of(d.time_hi.begin(), d.time_hi.end(), nonfinite)
        || std::any_of(d.time_lo.begin(), d.time_lo.end(), nonfinite)) {
        throw std::invalid_argument("Cannot invoke the propagate_until() function of an adaptive Taylor integrator "
                                    "in batch mode if one of the current times is not finite");
    }
    if (std::any_of(tf_hi.begin(), tf_hi.end(), nonfinite) || std::any_of(tf_lo.begin(), tf_lo.end(), nonfinite)) {
        throw std::invalid_argument("A non-finite time was passed to the propagate_until() function of an adaptive "
                                    "Taylor integrator in batch mode");
    }
    check_max_delta_ts(max_delta_ts, N, "propagate_until()");
    std::vector<dfloat> rem(N);
    for (std::uint32_t i = 0; i < N; ++i) {
        rem[i] = dfloat(tf_hi[i], tf_lo[i]) - dfloat(d.time_hi[i], d.time_lo[i]);
        if (!isfinite(rem[i])) {
            throw std::invalid_argument("The final time passed to the propagate_until() function of an adaptive "
                                        "Taylor integrator in batch mode results in an overflow condition");
        }
    }

    d.prop_res_override.reset();
    d.fix_step_limit = false;

    // The reference's batch-wide semantics (src/taylor_adaptive_batch.cpp:1404-1407, :1462-1467, :1516): a non-finite lane
    // stops the whole batch at that iteration, max_steps counts lock-step iterations of the batch and the lanes which are
    // done keep taking zero-length steps. batch_semantics = 1 routes propagate_until() / propagate_for() through the
    // lock-step loop (one step of every lane per sweep), which implements exactly that; the default (0) runs every lane's
    // own loop on the device and falls back to the lock-step loop only where the outcomes would differ (DESIGN.md,
    // "Outcome semantics").
    const bool ref_semantics = d.batch_semantics == 1 || d.force_lockstep;

    if (!cb && !c_out && !d.has_events() && !ref_semantics) {
        // Device-resident propagation: every lane runs its own adaptive loop to completion
        // (or to max_steps) inside a single kernel launch.
        d.before_kernel();
        d.d_tfhi.upload(tf_hi.data(), tf_hi.size() * sizeof(double), d.stream);
        d.d_tflo.upload(tf_lo.data(), tf_lo.size() * sizeof(double), d.stream);
        d.launch_propagate(*d.dmod, nullptr, max_delta_ts, max_steps, wtc);
        finish_device_propagate(ts_, max_steps, max_delta_ts, wtc);
        return;
    }

    // callback::angle_reducer alone, no continuous output, no events: the persistent kernel of the stepper variant which
    // reduces the flagged state variables of a system right after each of its state updates. Every system
    // takes at least one - possibly zero-length - step in the kernel, like in the reference's loop, hence every system is
    // reduced at least once. Step limits, outcomes, counters and the safety net of the default semantics are those of the
    // propagation without a callback; the re-run after a rollback goes through the lock-step loop with the callback.
    bool pre_done = false;
    if (cb && red && !c_out && !d.has_events() && !ref_semantics) {
        if (pre) {
            d.call_keeping_time("propagate_until()", pre);
        }
        pre_done = true;
        const auto idx = red();
        // (The pre_hook() has just rebuilt the indices from the system of this integrator: they fit it.)
        auto *var = idx.empty() ? nullptr : &d.get_ar_variant(idx);
        if (var != nullptr && var->cm) {
            detail::log_message(log_level::info, "propagate_until(): angle_reducer fused into the propagate kernel of the stepper ("
                                                     + get_codegen_info() + ")");
            d.before_kernel();
            if (!var->dm) {
                var->dm = std::make_unique<device_module>(var->cm, d.device);
            }
            var->dm->set_stream(d.stream);
            // (One final time for every lane travels as a kernel argument, per-lane ones as two arrays.)
            const bool scalar_tf = ts_.size() == 1u;
            if (!scalar_tf) {
                d.d_tfhi.upload(tf_hi.data(), tf_hi.size() * sizeof(double), d.stream);
                d.d_tflo.upload(tf_lo.data(), tf_lo.size() * sizeof(double), d.stream);
            }
            d.launch_propagate(*var->dm, scalar_tf ? &ts_[0] : nullptr, max_delta_ts, max_steps, wtc);
            d.last_cb_path = 3;
            finish_device_propagate(ts_, max_steps, max_delta_ts, wtc, cb);
            return;
        }
        detail::log_message(log_level::info,
                            "propagate_until(): angle_reducer applied by hy_angle_reduce after every sweep of the lock-step loop: "
                                + (var != nullptr ? var->why_not : std::string("no state variable of the system is reduced")));
    }

    // Lock-step propagation with a callback executed after every sweep and/or the recording of the
    // continuous output: the reference's loop, one single-step kernel launch per iteration.
    // The pre_hook() of the step callback, once, before the first step (src/taylor_adaptive_batch.cpp:1356-1365).
    if (cb) {
        d.last_cb_path = d.cb_is_library ? 4 : (d.cb_is_reducer ? 2 : 1);
        if (d.cb_is_library) {
            detail::log_message(log_level::info, "propagate_until(): library-side step callback (step_action) applied by its kernel after "
                                                 "every sweep of the lock-step loop: fusing it into the propagate kernel is not implemented");
        }
        if (d.cb_is_reducer && !pre_done && !d.force_lockstep) {
            detail::log_message(log_level::info,
                                "propagate_until(): angle_reducer applied by hy_angle_reduce after every sweep of the lock-step loop ("
                                    + std::string(c_out ? "continuous output" : (d.has_events() ? "events" : "lock-step semantics"))
                                    + ")");
        }
    }
    if (cb && pre && !pre_done) {
        d.call_keeping_time("propagate_until()", pre);
        // (The hook may have changed the state: the remaining times only depend on the times.)
    }
    // If c_out is true, we always need to write the Taylor coefficients (:1243-1244).
    wtc = wtc || c_out;
    std::unique_ptr<c_out_builder> cob;
    if (c_out) {
        d.ensure_device();
        cob = std::make_unique<c_out_builder>(N, d.order, d.dim, d.high_accuracy, d.device, d.stream, d.time_hi,
                                              d.time_lo);
    }
    std::vector<int> t_dir(N);
    std::vector<double> min_abs_h(N, std::numeric_limits<double>::infinity()), max_abs_h(N, 0.);
    std::vector<double> cur_max(N);
    for (std::uint32_t i = 0; i < N; ++i) {
        t_dir[i] = rem[i] >= dfloat(0.);
    }
    const auto pinf = std::numeric_limits<double>::infinity();
    std::size_t iter_counter = 0;

    // Device-driven loop: the per-lane bookkeeping runs in a post-step kernel, the host reads three counters per
    // sweep, runs the callback and (for the continuous output) appends the coefficients device-to-device.
    d.ensure_device();
    d.ensure_tc();
    d.ensure_grid_mod();
    const auto dsz = sizeof(double);
    device_buffer b_rem_hi(N * dsz, d.device), b_rem_lo(N * dsz, d.device), b_mdt(N * dsz, d.device);
    device_buffer b_tdir(N * sizeof(int), d.device), b_cnt(6u * sizeof(unsigned), d.device);
    std::vector<double> rhi(N), rlo(N), mdts(N);
    const std::vector<unsigned long long> ns0(N, 0u);
    for (std::uint32_t i = 0; i < N; ++i) {
        rhi[i] = rem[i].hi;
        rlo[i] = rem[i].lo;
        mdts[i] = max_delta_ts.empty() ? pinf : max_delta_ts[i];
        cur_max[i] = first_step_limit(rem[i], t_dir[i], mdts[i]);
    }
    b_rem_hi.upload(rhi.data(), N * dsz, d.stream);
    b_rem_lo.upload(rlo.data(), N * dsz, d.stream);
    b_mdt.upload(mdts.data(), N * dsz, d.stream);
    b_tdir.upload(t_dir.data(), N * sizeof(int), d.stream);
    d.d_tfhi.upload(tf_hi.data(), N * dsz, d.stream);
    d.d_tflo.upload(tf_lo.data(), N * dsz, d.stream);
    d.d_lim.upload(cur_max.data(), N * dsz, d.stream);
    d.d_lim_src = nullptr;
    d.d_minh.upload(min_abs_h.data(), N * dsz, d.stream);
    d.d_maxh.upload(max_abs_h.data(), N * dsz, d.stream);
    d.d_nsteps.upload(ns0.data(), N * sizeof(unsigned long long), d.stream);
    // (Continuous output consumes the Taylor coefficients of every step.)
    const scoped_value<bool> tc_guard(d.ev_all_tc, static_cast<bool>(cob));
    // (Independent semantics: a loop ended by max_steps / the callback overrides the outcomes of the systems which are
    // neither done nor retired only, see impl::sweep_ctx.)
    const auto sw = d.start_retirement();
    const auto finish = [&](const grid_kargs &a, std::optional<taylor_outcome> oc) {
        if (oc) {
            sw.override_rest(a, *oc);
        }
        d.log_sweep_loop("propagate_until()", iter_counter);
        if (cob) {
            d.last_c_out = cob->finish(t_dir);
        }
    };
    while (true) {
        d.take_sweep_step(nullptr, wtc);
        b_cnt.zero(d.stream);
        // (The final times are in the double-length grid row 0: grid = hi, out = lo.)
        grid_kargs a{.grid = d.d_tfhi.as<double>(), .out = d.d_tflo.as<double>(), .thi = d.d_thi.as<double>(),
                     .tlo = d.d_tlo.as<double>(), .last_h = d.d_lasth.as<double>(), .outcome = d.d_outcome.as<long long>(),
                     .rem_hi = b_rem_hi.as<double>(), .rem_lo = b_rem_lo.as<double>(), .mdt = b_mdt.as<double>(),
                     .t_dir = b_tdir.as<int>(), .lim = d.d_lim.as<double>(), .min_h = d.d_minh.as<double>(),
                     .max_h = d.d_maxh.as<double>(), .n_steps = d.d_nsteps.as<unsigned long long>(),
                     .counters = b_cnt.as<unsigned>(), .N = N};
        sw.fill(a);
        d.grid_mod->launch("hy_until_post", N, 256, a, d.stream);
        unsigned cnt[6] = {0, 0, 0, 0, 0, 0};
        sw.read_counters(b_cnt, cnt, 3u);
        // Outcomes of the last sweep + accumulated statistics: on the device.
        d.prop_res_dev_newer = true;
        d.step_res_dev_newer = true;
        if (cnt[1] != 0u) {
            finish(a, {});
            return;
        }
        if (cob) {
            d.times_to_host();
            d.ensure_tc_expanded();
            cob->append(d.d_tc.as<double>(), d.time_hi, d.time_lo);
        }
        ++iter_counter;
        if (cb && !d.call_keeping_time("propagate_until()", cb)) {
            finish(a, taylor_outcome::cb_stop);
            return;
        }
        // (cnt[2]: lanes stopped by a terminal event - the propagation of the whole batch ends, :1411, :1429. Independent
        // semantics: they were retired, and counted in cnt[0].)
        if (cnt[0] == N || (!sw.indep && cnt[2] != 0u)) {
            finish(a, {});
            return;
        }
        if (iter_counter == max_steps) {
            finish(a, taylor_outcome::step_limit);
            return;
        }
    }
}

std::optional<c_out_core> tab_core::take_c_output()
{
    auto ret = std::move(m_impl->last_c_out);
    m_impl->last_c_out.reset();
    return ret;
}

void tab_core::propagate_grid_device_loop(const std::vector<double> &grid, std::vector<double> &retval,
                                          const std::vector<dfloat> &rem, const std::vector<int> &t_dir,
                                          const std::vector<double> &max_delta_ts, const grid_call &call)
{
    const auto max_steps = call.max_steps;
    double *const d_out = call.d_out;
    const auto &cb = call.hooks.call;
    const auto &stats = call.sampling.statistics;
    auto &d = *m_impl;
    const auto N = d.N;
    const auto dim = d.dim;
    const auto n_grid = static_cast<std::uint32_t>(grid.size() / N);
    const auto pinf = std::numeric_limits<double>::infinity();
    const auto dsz = sizeof(double);

    const auto stat_names = [](const std::vector<grid_statistic> &v) {
        std::string ret;
        for (const auto s : v) {
            ret += (ret.empty() ? "" : ", ") + std::string(grid_statistic_names[static_cast<int>(s)]);
        }
        return ret;
    };

    d.ensure_device();
    d.ensure_tc();
    d.ensure_grid_mod();
    // Grid observables: the post-step module with their section takes the place of the plain one for the
    // samples - hy_grid_post, hy_grid_unsample, and hy_grid_obs0 for row 0 -, one column per observable.
    // Grid statistics: the variant of that module which folds. Its output buffer holds the accumulators of the
    // lanes, n_slots * N doubles with those of the result first, and their shadow copy behind them - whatever the caller gets,
    // host vector or device buffer, is the first n_obs * n_stat * N of them, copied at the end.
    auto *const gov = call.sampling.observables ? &d.get_go_module(call.sampling) : nullptr;
    const bool folds = stats.has_value();
    const std::size_t n_res = folds ? gov->sec.n_obs * stats->size() * N : 0u;
    // Ensemble statistics: the variant which merges into the records of the grid points, n_grid * n_obs records
    // of ens_rec.words 64-bit words whatever the number of systems, with a copy of the same size behind them: the records
    // as they were before the samples of a sweep which may be taken back.
    // Ensemble histograms, alone or with the ensemble statistics: n_grid records of hist.words counters behind
    // the records above, the copy covers both, and the edge tables - data of the call, not of the module - follow the copy.
    // `ens` below is "the module merges into records": ens_words counts the words of both regions.
    const bool with_ens = call.sampling.ensemble.has_value(), with_hist = call.sampling.histograms.has_value();
    const bool ens = with_ens || with_hist;
    const std::size_t ens_only_words = with_ens ? static_cast<std::size_t>(n_grid) * gov->sec.n_obs * gov->sec.ens_rec.words : 0u;
    const std::size_t hist_words = with_hist ? static_cast<std::size_t>(n_grid) * gov->sec.hist.words : 0u;
    const std::size_t ens_words = ens_only_words + hist_words;
    auto ens_start = with_ens ? ens_init(gov->sec.ens_rec, static_cast<std::size_t>(n_grid) * gov->sec.n_obs) : std::vector<std::uint64_t>{};
    ens_start.resize(ens_words, 0u);
    const auto hist_edges = with_hist ? hist_edge_table(*call.sampling.histograms) : std::vector<double>{};
    aux_module &sample_mod = gov != nullptr ? gov->loaded(d.device) : *d.grid_mod;
    const std::size_t n_col = gov != nullptr ? gov->sec.n_obs : dim;
    device_buffer b_stage((gov != nullptr && gov->sec.staged) ? static_cast<std::size_t>(dim) * N * dsz : 0u, d.device);

    const auto out_doubles = ens ? 2u * ens_words + hist_edges.size() : (folds ? 2u * gov->sec.n_slots * static_cast<std::size_t>(N) : grid.size() * n_col);
    const bool own_out = folds || ens;
    device_buffer b_grid(grid.size() * dsz, d.device), b_out((d_out != nullptr && !own_out) ? 0u : out_doubles * dsz, d.device);
    double *const out_ptr = (d_out != nullptr && !own_out) ? d_out : b_out.as<double>();
    device_buffer b_rem_hi(N * dsz, d.device), b_rem_lo(N * dsz, d.device), b_mdt(N * dsz, d.device);
    device_buffer b_tdir(N * sizeof(int), d.device), b_gidx(N * sizeof(unsigned), d.device), b_cnt(6u * sizeof(unsigned), d.device),
        b_gidx_prev(N * sizeof(unsigned), d.device);
    b_grid.upload(grid.data(), grid.size() * dsz, d.stream);
    if (with_hist) {
        device_copy(b_out.as<double>() + 2u * ens_words, hist_edges.data(), hist_edges.size() * dsz, d.device, d.stream);
    }
    std::vector<double> rhi(N), rlo(N), lim(N), mn(N, pinf), mx(N, 0.), tg(N);
    std::vector<unsigned> gidx(N, 1u);
    std::vector<unsigned long long> ns(N, 0u);
    for (std::uint32_t i = 0; i < N; ++i) {
        rhi[i] = rem[i].hi;
        rlo[i] = rem[i].lo;
        lim[i] = first_step_limit(rem[i], t_dir[i], max_delta_ts[i]);
        tg[i] = n_grid > 1u ? grid[static_cast<std::size_t>(N) + i] : 0.;
    }
    b_mdt.upload(max_delta_ts.data(), N * dsz, d.stream);
    b_tdir.upload(t_dir.data(), N * sizeof(int), d.stream);
    device_buffer b_next_tg(N * dsz, d.device);
    // The samples and the per-lane bookkeeping at the first grid point: at the start, and again after a rollback (below).
    const auto init_grid_state = [&]() {
        // Row 0 = current state, everything else NaN until reached. (Statistics: hy_grid_obs0 below writes every accumulator.)
        if (ens) {
            // (The records in their start state; hy_grid_obs0 below merges row 0.)
            b_out.upload(ens_start.data(), ens_words * dsz, d.stream);
            if (d_out != nullptr) {
                d.to_device();
            }
        } else if (folds) {
            if (d_out != nullptr) {
                d.to_device();
            }
        } else if (d_out == nullptr) {
            b_out.upload(retval.data(), retval.size() * dsz, d.stream);
        } else {
            // NOTE: the all-ones byte pattern is a (quiet) NaN.
            device_fill_bytes(out_ptr, 0xFF, out_doubles * dsz, d.device, d.stream);
            d.to_device();
            if (gov == nullptr) {
                device_copy(out_ptr, d.d_state.get(), static_cast<std::size_t>(dim) * N * dsz, d.device, d.stream);
            }
        }
        if (gov != nullptr) {
            // (Row 0: the observables of the current state - the one the call without observables copies - at the first
            // grid time. The host output arrives all NaN.)
            d.before_kernel();
            const grid_kargs a0{.grid = b_grid.as<double>(), .out = out_ptr, .N = N, .n_grid = n_grid, .pars = d.d_pars.as<double>(),
                                .stage = b_stage.as<double>(), .state = d.d_state.as<double>()};
            sample_mod.launch("hy_grid_obs0", N, 256, a0, d.stream);
        }
        b_rem_hi.upload(rhi.data(), N * dsz, d.stream);
        b_rem_lo.upload(rlo.data(), N * dsz, d.stream);
        b_gidx.upload(gidx.data(), N * sizeof(unsigned), d.stream);
        d.d_lim.upload(lim.data(), N * dsz, d.stream);
        d.d_lim_src = nullptr;
        d.d_minh.upload(mn.data(), N * dsz, d.stream);
        d.d_maxh.upload(mx.data(), N * dsz, d.stream);
        d.d_nsteps.upload(ns.data(), N * sizeof(unsigned long long), d.stream);
        b_next_tg.upload(tg.data(), N * dsz, d.stream);
    };
    init_grid_state();

    d.prop_res_override.reset();
    d.fix_step_limit = false;
    std::size_t iter_counter = 0;
    bool any_step = false;
    // Taylor coefficients on demand: dense output is evaluated only in the steps which reach a grid point, so a stepper
    // which can tell (emitted_module::tc_by_threshold) stores the coefficients of those steps only - unless a step callback
    // may look at them, or the stepper with events is in charge (its own on-demand logic is switched off below).
    const bool tc_on_demand = !cb && !d.has_events() && d.emitted.tc_by_threshold && n_grid > 1u;
    // From grid point to grid point in ONE launch per lane (emitted_module::grid_multi_step, hy_kargs::tc_thr): without a
    // callback and without events nothing happens on the host between two sweeps, and the lanes are independent - every lane
    // runs its own steps inside a propagate-mode launch until the step which reaches its next grid time, whose coefficients
    // it stores; hy_grid_post then evaluates the dense output of that step. A launch per grid interval instead of a launch
    // per step: the lock-step loop was at 0.7 of the rate of the propagation loop (ramp-up / drain and clock of 2-ms
    // launches). max_steps counts lock-step iterations of the batch: with a step limit the single-step sweeps stay.
    // With the reference's semantics (batch_semantics == 0) a lane which goes non-finite stops the whole batch after THAT
    // sweep (src/taylor_adaptive_batch.cpp:1936-2000), i.e. after the same number of steps in every lane. The launches
    // take every lane to its own grid crossing - after a few launches the lanes have taken different numbers of steps -, so
    // a launch in which a lane goes non-finite sends the whole call back to the snapshot taken before the FIRST launch
    // (state, times; samples and per-lane bookkeeping from the host; hy_grid_post records nothing of that launch), and the
    // grid is redone from its start in single-step sweeps. batch_semantics == 2 keeps the per-lane behaviour.
    bool multi_step = tc_on_demand && d.emitted.grid_multi_step && max_steps == 0u && d.batch_semantics != 1;
    const bool multi_step_chosen = multi_step;
    std::size_t n_launches = 0, n_rollbacks = 0;
    device_buffer b_acc_ns(multi_step ? N * sizeof(unsigned long long) : 0u, d.device), b_acc_min(multi_step ? N * dsz : 0u, d.device),
        b_acc_max(multi_step ? N * dsz : 0u, d.device), b_grid_done(multi_step ? N * dsz : 0u, d.device);
    if (multi_step) {
        std::vector<double> tl(N), zero(N, 0.);
        for (std::uint32_t i = 0; i < N; ++i) {
            tl[i] = grid[static_cast<std::size_t>(n_grid - 1u) * N + i];
        }
        d.d_tfhi.upload(tl.data(), N * dsz, d.stream);
        d.d_tflo.upload(zero.data(), N * dsz, d.stream);
        b_acc_ns.upload(ns.data(), N * sizeof(unsigned long long), d.stream);
        b_acc_min.upload(mn.data(), N * dsz, d.stream);
        b_acc_max.upload(mx.data(), N * dsz, d.stream);
        if (d.batch_semantics == 0) {
            d.before_kernel();
            d.snapshot_for_rollback();
        }
    }
    const scoped_value<const double *> thr_guard(d.tc_threshold, tc_on_demand ? b_next_tg.as<double>() : nullptr);
    // (The dense output over the grid consumes the Taylor coefficients of every step.)
    const scoped_value<bool> tc_guard(d.ev_all_tc, true);
    d.tc_stale = false;
    // Independent semantics: see the loop of propagate_until(). A retired system keeps the samples of its last step, its
    // remaining rows stay NaN and its grid index goes to the end (hy_grid_post).
    const auto sw = d.start_retirement();
    // (A system retired by a step_action is through its grid.)
    const scoped_value<unsigned *> sa_gidx_guard(d.sa_gidx, b_gidx.as<unsigned>());
    const scoped_value<unsigned> sa_ngrid_guard(d.sa_n_grid, n_grid);
    while (n_grid > 1u) {
        // (The sweep after which max_steps ends the loop stores the coefficients of EVERY lane: the reference leaves the
        // Taylor coefficients of the last step behind, src/taylor_adaptive_batch.cpp:1546-2055.)
        if (tc_on_demand && max_steps != 0u && iter_counter + 1u == max_steps) {
            d.tc_threshold = nullptr;
        }
        if (multi_step) {
            d.before_kernel();
            d.d_counters.zero(d.stream);
            auto ka = d.base_args();
            ka.tfin_hi = d.d_tfhi.as<double>();
            ka.tfin_lo = d.d_tflo.as<double>();
            ka.lim = b_mdt.as<double>();
            ka.tc = d.d_tc.as<double>();
            ka.tc_thr = b_next_tg.as<double>();
            ka.grid_done = b_grid_done.as<double>();
            ka.mode = 1;
            ka.pad = 4;
            ka.max_steps = 0;
            d.dmod->launch_taylor(ka);
            d.after_kernel(true);
            d.step_res_dev_newer = true;
        } else {
            d.take_sweep_step(nullptr, true);
        }
        ++n_launches;
        any_step = true;
        d.ensure_tc_expanded();
        b_cnt.zero(d.stream);
        grid_kargs a{.grid = b_grid.as<double>(), .out = out_ptr, .tc = d.d_tc.as<double>(), .thi = d.d_thi.as<double>(),
                     .tlo = d.d_tlo.as<double>(), .last_h = d.d_lasth.as<double>(), .outcome = d.d_outcome.as<long long>(),
                     .rem_hi = b_rem_hi.as<double>(), .rem_lo = b_rem_lo.as<double>(), .mdt = b_mdt.as<double>(),
                     .t_dir = b_tdir.as<int>(), .lim = d.d_lim.as<double>(), .gidx = b_gidx.as<unsigned>(),
                     .min_h = d.d_minh.as<double>(), .max_h = d.d_maxh.as<double>(),
                     .n_steps = d.d_nsteps.as<unsigned long long>(), .counters = b_cnt.as<unsigned>(), .N = N, .n_grid = n_grid,
                     .next_tg = tc_on_demand ? b_next_tg.as<double>() : nullptr,
                     .acc_n_steps = multi_step ? b_acc_ns.as<unsigned long long>() : nullptr,
                     .acc_min_h = multi_step ? b_acc_min.as<double>() : nullptr,
                     .acc_max_h = multi_step ? b_acc_max.as<double>() : nullptr,
                     .grid_done = multi_step ? b_grid_done.as<double>() : nullptr,
                     .launch_nf = (multi_step && d.batch_semantics == 0) ? d.d_counters.as<unsigned>() : nullptr,
                     .gidx_prev = b_gidx_prev.as<unsigned>()};
        if (gov != nullptr) {
            a.pars = d.d_pars.as<double>();
            a.stage = b_stage.as<double>();
        }
        sw.fill(a);
        if (ens && !multi_step) {
            // (A single-step sweep may take its samples back: all of them, so all the records as they are now.)
            device_copy(b_out.as<double>() + ens_words, b_out.get(), ens_words * dsz, d.device, d.stream);
        }
        sample_mod.launch("hy_grid_post", N, 256, a, d.stream);
        unsigned cnt[6] = {0, 0, 0, 0, 0, 0};
        sw.read_counters(b_cnt, cnt, 4u);
        if (cnt[3] != 0u) {
            // A lane went non-finite inside a multi-step launch: back to the start of the grid, and all of it again in
            // single-step sweeps.
            d.rollback_to_snapshot();
            init_grid_state();
            iter_counter = 0;
            multi_step = false;
            ++n_rollbacks;
            continue;
        }
        if (cnt[1] != 0u) {
            // (Lock-step sweeps: no samples of this step, src/taylor_adaptive_batch.cpp:1962-1968. The multi-step launches of
            // batch_semantics == 2 keep theirs: every lane on its own.)
            if (!multi_step) {
                if (ens) {
                    device_copy(b_out.get(), b_out.as<double>() + ens_words, ens_words * dsz, d.device, d.stream);
                } else {
                    sample_mod.launch("hy_grid_unsample", N, 256, a, d.stream);
                }
            }
            // A non-finite state was detected: stop (the outcomes of the last step are reported). With coefficients on
            // demand the lanes which did not reach a grid point in this sweep hold the coefficients of OLDER steps:
            // get_tc() / update_d_output() refuse to hand those out as the last step's (tc_stale).
            d.tc_stale = tc_on_demand && d.tc_threshold != nullptr;
            break;
        }
        ++iter_counter;
        if (cb) {
            // The step callback, once per sweep (src/taylor_adaptive_batch.cpp:2003-2040); it may read or write the state
            // through the lazily synchronised mirrors, but not move the time coordinate (generation counter).
            d.prop_res_dev_newer = true;
            d.step_res_dev_newer = true;
            if (!d.call_keeping_time("propagate_grid()", cb)) {
                // (The systems which are neither through their grid nor retired: here and with max_steps below.)
                sw.override_rest(a, taylor_outcome::cb_stop);
                break;
            }
        }
        // (cnt[2]: lanes stopped by a terminal event - they interrupt the propagation of the whole batch. Independent
        // semantics: they were retired, their grid index is at the end.)
        if (cnt[0] == 0u || (!sw.indep && cnt[2] != 0u)) {
            break;
        }
        if (iter_counter == max_steps) {
            sw.override_rest(a, taylor_outcome::step_limit);
            break;
        }
    }
    d.log_sweep_loop("propagate_grid()", iter_counter);
    if (detail::log_enabled(log_level::debug)) {
        detail::log_message(
            log_level::debug,
            std::string("propagate_grid() loop: ")
                + (multi_step_chosen ? "multi-step launches (one per grid interval and lane: no callback, no events, no "
                                       "max_steps, Taylor coefficients on demand)"
                                     : (!tc_on_demand ? "single-step sweeps (a callback, events or a single grid point: "
                                                        "the coefficients of every step)"
                                                      : "single-step sweeps (the stepper has no multi-step grid mode, "
                                                        "max_steps > 0 or lock-step semantics)"))
                + ", " + std::to_string(n_launches) + " stepper launches for " + std::to_string(n_grid - 1u)
                + " grid intervals"
                + (n_rollbacks != 0u ? ", a non-finite lane: rolled back to the start of the grid and redone in single-step sweeps"
                                     : "")
                + (gov != nullptr ? ", " + std::to_string(gov->sec.n_obs) + " observables over " + std::to_string(gov->sec.reads.size())
                                        + " of " + std::to_string(dim) + " state rows, samples held "
                                        + (gov->sec.staged ? "in the staging buffer" : "in registers")
                                  : std::string{})
                + (folds ? ", statistics " + stat_names(*stats) + " folded over the grid (" + std::to_string(gov->sec.n_slots)
                               + " accumulators per system)"
                         : std::string{})
                + (with_ens ? ", ensemble statistics merged across the systems per grid point (" + std::to_string(gov->sec.ens_rec.words)
                                  + " words per grid point and observable, "
                                  + (gov->sec.ens_aggregate ? "aggregated per wavefront" : "one atomic per lane") + ")"
                            : std::string{})
                + (with_hist ? ", ensemble histograms counted across the systems per grid point (" + std::to_string(gov->sec.hist.words)
                                   + " words per grid point, merge mode "
                                   + hist_mode_names[static_cast<int>(gov->sec.hist_merge_mode)]
                                   + (gov->sec.hist_merge_mode == hist_mode::hybrid
                                          ? " of " + std::to_string(gov->sec.hist_turns) + " turns"
                                          : std::string{})
                                   + ")"
                             : std::string{}));
    }
    if (multi_step && any_step) {
        // (The accumulated counters / extrema take the place of the last launch's own.)
        device_copy(d.d_nsteps.get(), b_acc_ns.get(), N * sizeof(unsigned long long), d.device, d.stream);
        device_copy(d.d_minh.get(), b_acc_min.get(), N * dsz, d.device, d.stream);
        device_copy(d.d_maxh.get(), b_acc_max.get(), N * dsz, d.device, d.stream);
    }
    if (any_step) {
        // Outcomes of the last sweep + the accumulated statistics live on the device.
        d.prop_res_dev_newer = true;
        d.step_res_dev_newer = true;
    }
    if (ens) {
        // The records to the caller: the words to the device buffer or to grid_call::ens_raw, their values to retval.
        std::vector<std::uint64_t> raw(ens_words);
        b_out.download(raw.data(), ens_words * dsz, d.stream);
        if (d_out != nullptr) {
            device_copy(d_out, b_out.get(), ens_words * dsz, d.device, d.stream);
            stream_synchronize(d.device, d.stream);
        }
        give_records(gov->sec, call, std::move(raw), ens_only_words, d_out == nullptr ? &retval : nullptr);
    } else if (folds && d_out != nullptr) {
        device_copy(d_out, b_out.get(), n_res * dsz, d.device, d.stream);
        stream_synchronize(d.device, d.stream);
    } else if (d_out == nullptr) {
        b_out.download(retval.data(), retval.size() * dsz, d.stream);
    } else {
        stream_synchronize(d.device, d.stream);
    }
}

// Reference: propagate_grid_impl(), src/taylor_adaptive_batch.cpp:1546-2055. Host-driven lock-step loop:
// single-step kernel launches (always with the Taylor coefficients) interleaved with dense-output launches.
// grid[point * N + lane]; return value ret[(point * dim + var) * N + lane], NaN where not reached.
std::vector<double> tab_core::propagate_grid(std::vector<double> grid, const grid_call &call)
{
    const auto max_steps = call.max_steps;
    const auto &max_delta_ts_ = call.max_delta_ts;
    double *const d_out = call.d_out;
    const auto &[cb, pre, red, lib_cb] = call.hooks;
    const auto &stats = call.sampling.statistics;
    const bool with_obs = call.sampling.observables.has_value();
    auto &d = *m_impl;
    const auto N = d.N;
    const auto dim = d.dim;
    const auto pinf = std::numeric_limits<double>::infinity();

    // Grid observables: the checks against the system before anything runs; n_col columns per grid point.
    // (... and the statistics: retval is the reduced output, NaN and a count of zero until the loop has run.)
    const std::size_t n_col = with_obs ? d.get_go_module(call.sampling).sec.n_obs : dim;

    if (grid.empty()) {
        throw std::invalid_argument(
            "Cannot invoke propagate_grid() in an adaptive Taylor integrator in batch mode if the time grid is empty");
    }
    if (grid.size() % N != 0u) {
        throw std::invalid_argument("Invalid grid size detected in propagate_grid() for an adaptive Taylor integrator "
                                    "in batch mode: the grid has a size of "
                                    + std::to_string(grid.size()) + ", which is not a multiple of the batch size ("
                                    + std::to_string(N) + ")");
    }
    // The current time coordinates (src/taylor_adaptive_batch.cpp:1588-1593).
    d.times_to_host();
    if (std::any_of(d.time_hi.begin(), d.time_hi.end(), [](double t) { return !std::isfinite(t); })
        || std::any_of(d.time_lo.begin(), d.time_lo.end(), [](double t) { return !std::isfinite(t); })) {
        throw std::invalid_argument("Cannot invoke propagate_grid() in an adaptive Taylor integrator in batch mode if "
                                    "the current time is not finite");
    }
    const std::vector<double> max_delta_ts = max_delta_ts_.empty() ? std::vector<double>(N, pinf) : max_delta_ts_;
    check_max_delta_ts(max_delta_ts, N, "propagate_grid()");

    const auto n_grid_points = grid.size() / N;
    const auto *const gp = grid.data();
    const auto is_nf = [](double t) { return !std::isfinite(t); };
    const char *nf_err_msg
        = "A non-finite time value was passed to propagate_grid() in an adaptive Taylor integrator in batch mode";
    const char *ig_err_msg = "A non-monotonic time grid was passed to propagate_grid() in an adaptive "
                             "Taylor integrator in batch mode";
    if (std::any_of(gp, gp + N, is_nf)) {
        throw std::invalid_argument(nf_err_msg);
    }
    if (n_grid_points > 1u) {
        if (std::any_of(gp + N, gp + 2u * N, is_nf)) {
            throw std::invalid_argument(nf_err_msg);
        }
        if (gp[N] == gp[0]) {
            throw std::invalid_argument(ig_err_msg);
        }
        const auto grid_direction = gp[N] > gp[0];
        for (std::uint32_t i = 1; i < N; ++i) {
            if ((gp[N + i] > gp[i]) != grid_direction) {
                throw std::invalid_argument(ig_err_msg);
            }
        }
        // (Row by row: finiteness of the whole row first, then the ordering - src/taylor_adaptive_batch.cpp:1652-1661.)
        for (std::size_t k = 2; k < n_grid_points; ++k) {
            if (std::any_of(gp + k * N, gp + (k + 1u) * N, is_nf)) {
                throw std::invalid_argument(nf_err_msg);
            }
            for (std::uint32_t i = 0; i < N; ++i) {
                if ((gp[k * N + i] > gp[(k - 1u) * N + i]) != grid_direction) {
                    throw std::invalid_argument(ig_err_msg);
                }
            }
        }
    }
    d.to_host();
    for (std::uint32_t i = 0; i < N; ++i) {
        if (d.time_hi[i] != gp[i]) {
            throw std::invalid_argument("When invoking propagate_grid(), the first element of the time grid "
                                        "must match the current time coordinate - however, the first element of the "
                                        "time grid at batch index "
                                        + std::to_string(i) + " has a value of " + fp_to_string(gp[i])
                                        + ", while the current time coordinate is " + fp_to_string(d.time_hi[i]));
        }
    }

    // NOTE: with a caller-provided device output (MI355X extension, no callback) nothing of size n_grid * dim * N
    // is ever materialised on the host: the samples go straight to d_out and an empty vector is returned.
    if (d_out != nullptr && cb) {
        throw std::invalid_argument("propagate_grid() with a device output buffer does not support callbacks");
    }
    const auto &ens = call.sampling.ensemble;
    const auto &hist = call.sampling.histograms;
    // (Ensemble statistics and histograms: the values of the former, then the counters of the latter as doubles.)
    const std::size_t n_rec_vals = (ens ? grid.size() / N * n_col * ens->size() : 0u)
                                   + (hist ? grid.size() / N * d.get_go_module(call.sampling).sec.hist.words : 0u);
    std::vector<double> retval(d_out != nullptr
                                   ? 0u
                                   : ((ens || hist) ? n_rec_vals : (stats ? n_col * stats->size() * N : grid.size() * n_col)),
                               std::numeric_limits<double>::quiet_NaN());
    if (ens || hist) {
        // (Ensemble statistics, histograms: until the loop has run, the records in their start state - nothing was merged.)
        const auto &sec = d.get_go_module(call.sampling).sec;
        const auto n_rec = grid.size() / N * n_col;
        auto start = ens ? ens_init(sec.ens_rec, n_rec) : std::vector<std::uint64_t>{};
        const auto ens_words = start.size();
        start.resize(ens_words + grid.size() / N * sec.hist.words, 0u);
        if (d_out != nullptr) {
            d.ensure_device();
            device_copy(d_out, start.data(), start.size() * sizeof(std::uint64_t), d.device, d.stream);
            stream_synchronize(d.device, d.stream);
        }
        give_records(sec, call, std::move(start), ens_words, d_out == nullptr ? &retval : nullptr);
    }
    if (stats && d_out == nullptr) {
        for (std::size_t k = 0; k < stats->size(); ++k) {
            if ((*stats)[k] == grid_statistic::count) {
                for (std::size_t o = 0; o < n_col; ++o) {
                    std::fill_n(retval.begin() + static_cast<std::ptrdiff_t>((o * stats->size() + k) * N), N, 0.);
                }
            }
        }
    }
    std::vector<double> pgrid_tmp(gp, gp + N);

    // Propagate up to the first grid point (absorbs the low part of the double-length time).
    propagate_until(pgrid_tmp, max_steps, max_delta_ts, step_hooks{}, true, false);
    d.fetch_prop_res();
    if (std::any_of(d.prop_res.begin(), d.prop_res.end(),
                    [](const auto &t) { return std::get<0>(t) != taylor_outcome::time_limit; })) {
        for (auto &[oc, min_h, max_h, ts_count] : d.prop_res) {
            (void)oc;
            min_h = pinf;
            max_h = 0;
            ts_count = 0;
        }
        return retval;
    }
    if (d_out == nullptr) {
        d.to_host();
        // (With observables row 0 is computed on the device, hy_grid_obs0.)
        if (!with_obs) {
            std::copy(d.state.begin(), d.state.end(), retval.begin());
        }
    } else {
        d.times_to_host();
    }

    std::vector<dfloat> rem(N), t0(N), t1(N);
    std::vector<int> t_dir(N);
    for (std::uint32_t i = 0; i < N; ++i) {
        rem[i] = dfloat(gp[(n_grid_points - 1u) * N + i]) - dfloat(d.time_hi[i], d.time_lo[i]);
        if (!isfinite(rem[i])) {
            throw std::invalid_argument("The final time passed to the propagate_grid() function of an adaptive Taylor "
                                        "integrator in batch mode results in an overflow condition");
        }
        t_dir[i] = rem[i] >= dfloat(0.);
    }

    // The pre_hook() of the step callback (src/taylor_adaptive_batch.cpp:1782-1791).
    if (cb && pre) {
        d.call_keeping_time("propagate_grid()", pre);
    }
    // Device-resident lock-step loop: the step kernel and a post-step kernel (bookkeeping of the reference's loop, dense
    // output at the grid points covered by the step, next step limit) alternate without any per-lane host work; the host
    // reads three counters per sweep and runs the callback, if any.
    // (A pure angle_reducer callback runs hy_angle_reduce after every sweep: no fused grid launches.)
    d.cb_is_library = cb && lib_cb;
    d.last_cb_path = cb ? (d.cb_is_library ? 4 : (red ? 2 : 1)) : 0;
    propagate_grid_device_loop(grid, retval, rem, t_dir, max_delta_ts, call);
    return retval;
}

// ---- grid observables and statistics ----
void tab_core::prepare_grid_sampling(const grid_sampling &gs)
{
    if (gs.observables) {
        (void)m_impl->get_go_module(gs);
    }
}

tab_core::module_view tab_core::grid_sampling_module(const grid_sampling &gs)
{
    const auto &m = m_impl->get_go_module(gs);
    return {m.source, m.cm->code};
}

// ---- callback::angle_reducer ----
void tab_core::angle_reduce(const std::vector<std::uint32_t> &idx)
{
    auto &d = *m_impl;
    if (idx.empty()) {
        return;
    }
    if (!std::is_sorted(idx.begin(), idx.end()) || idx.back() >= d.dim) {
        throw std::invalid_argument("Invalid list of state variables passed to the angle reduction of an adaptive Taylor "
                                    "integrator in batch mode");
    }
    if (d.sticky_host_ptr || d.host_newer || !d.dmod) {
        // The host mirror is the newer copy (or a mutable pointer to it is out, and it is refreshed after every launch and
        // uploaded before the next one anyway): reduce it in place.
        d.to_host();
        for (const auto i : idx) {
            auto *row = d.state.data() + static_cast<std::size_t>(i) * d.N;
            for (std::uint32_t s = 0; s < d.N; ++s) {
                row[s] = angle_reduce_host(row[s]);
            }
        }
        d.host_newer = true;
        return;
    }
    if (!d.ar_mod) {
        d.ar_mod = std::make_unique<aux_module>(hiprtc_compile_source(make_angle_reduce_source()), d.device);
    }
    if (idx != d.ar_idx_dev) {
        d.d_ar_idx = device_buffer(idx.size() * sizeof(std::uint32_t), d.device);
        d.ar_idx_dev = idx;
        d.d_ar_idx.upload(d.ar_idx_dev.data(), d.ar_idx_dev.size() * sizeof(std::uint32_t), d.stream);
    }
    const ar_kargs a{d.d_state.as<double>(), d.d_ar_idx.as<unsigned>(), d.N, static_cast<unsigned>(idx.size())};
    d.ar_mod->launch("hy_angle_reduce", static_cast<std::uint64_t>(d.N) * idx.size(), 256, a, d.stream);
    // The device copy of the state is the newer one; callers who hold references to the host mirror see it refreshed.
    d.dev_newer = true;
    if (d.sticky_const_refs) {
        d.to_host();
    }
}

// ---- step_action ----
bool tab_core::apply_step_action(const step_action &act)
{
    auto &d = *m_impl;
    // (The checks against the system, the first time; the kernel from then on.)
    auto &var = d.get_sa_module(act);
    // The state is never downloaded: when the host mirror is the newer copy (or a mutable pointer to it is out) it is
    // uploaded first, like before any kernel. A device which has not run a step yet holds no last_h: the mirror's.
    const bool fresh_device = !d.dmod;
    const bool upload = d.host_newer || d.sticky_host_ptr || fresh_device;
    if (fresh_device || !d.lasth_dev_newer) {
        // (No step since the mirror of last_h was made current - a fresh integrator, a copy, a move to another device: the
        // device array may never have been written.)
        (void)get_last_h();
        if (std::all_of(d.last_h.begin(), d.last_h.end(), [](double h) { return h == 0.; })) {
            detail::log_message(log_level::debug, "step_action: no system has taken a step of non-zero length, nothing to do");
            return true;
        }
    }
    d.before_kernel();
    if (fresh_device || !d.lasth_dev_newer) {
        d.d_lasth.upload(d.last_h.data(), d.last_h.size() * sizeof(double), d.stream);
    }
    if (detail::log_enabled(log_level::debug)) {
        detail::log_message(log_level::debug, std::string("step_action: kernel hy_step_action over the device-resident state (")
                                                  + (upload ? "the host mirror was the newer copy: uploaded first"
                                                            : "the device copy was current: nothing moved")
                                                  + ")");
    }
    auto &mod = var.loaded(d.device);
    const bool cond = var.sec.has_cond;
    const bool indep = cond && d.retired_ptr != nullptr;
    if (cond) {
        if (d.d_sa_cnt.bytes() == 0u) {
            d.d_sa_cnt = device_buffer(sizeof(unsigned), d.device);
        }
        d.d_sa_cnt.zero(d.stream);
    }
    const sa_kargs a{d.d_lasth.as<double>(),
                     d.d_state.as<double>(),
                     d.d_pars.as<double>(),
                     d.d_thi.as<double>(),
                     cond ? d.d_sa_cnt.as<unsigned>() : nullptr,
                     indep ? d.d_retired.as<long long>() : nullptr,
                     indep ? d.d_outcome.as<long long>() : nullptr,
                     indep ? d.d_lim.as<double>() : nullptr,
                     indep ? d.sa_gidx : nullptr,
                     d.N,
                     d.sa_n_grid,
                     0u};
    if (d.ev_timing) {
        d.sa_ms += mod.launch_timed("hy_step_action", d.N, 256, a, d.stream);
        ++d.sa_timed;
    } else {
        mod.launch("hy_step_action", d.N, 256, a, d.stream);
    }
    // The device copy of the state is the newer one; the mirrors somebody holds follow, as after any kernel.
    d.dev_newer = true;
    d.refresh_held_mirrors();
    if (!cond) {
        return true;
    }
    unsigned n_stop = 0;
    d.d_sa_cnt.download(&n_stop, sizeof(unsigned), d.stream);
    if (indep) {
        // (The systems were retired on their own: the loop carries on.)
        d.n_stopped_by_action += n_stop;
        return true;
    }
    return n_stop == 0u;
}

void tab_core::prepare_step_action(const step_action &act)
{
    (void)m_impl->get_sa_module(act);
}

std::uint64_t tab_core::get_n_stopped_by_action() const
{
    return m_impl->n_stopped_by_action;
}

tab_core::module_view tab_core::step_action_module(const step_action &act)
{
    const auto &m = m_impl->get_sa_module(act);
    return {m.source, m.cm->code};
}

std::pair<double, std::uint64_t> tab_core::get_step_action_kernel_ms() const
{
    return {m_impl->sa_ms, m_impl->sa_timed};
}

int tab_core::get_last_callback_path() const
{
    return m_impl->last_cb_path;
}

std::string tab_core::get_angle_reduce_variant_source(const std::vector<std::uint32_t> &idx, std::string &why_not) const
{
    auto o = m_impl->eo;
    o.angle_reduce = idx;
    return emit_angle_reduce_variant(m_impl->prog, o, why_not).source;
}

double tab_core::get_angle_reduce_compile_seconds() const
{
    return m_impl->ar_compile_seconds;
}

} // namespace heyoka_amd::detail
