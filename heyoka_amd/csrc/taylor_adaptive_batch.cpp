// Host driver of the MI355X batch Taylor integrator. See taylor_adaptive_batch.hpp. Construction, mirrors, getters and
// setters, device move and the raw stepper ABI; the event step is in tab_events.cpp, the propagate_*() loops in
// tab_propagate.cpp, the post-step kernels in grid_post.cpp.
#include "tab_impl.hpp"

namespace heyoka_amd::detail
{

namespace
{

// Code generator from the configuration field (0 automatic: the wave-cluster generator is tried first and falls back
// by itself, see emit_hip_module()).
emit_mode choose_mode(int emitter)
{
    switch (emitter) {
        case 1:
            return emit_mode::unrolled;
        case 3:
            return emit_mode::table;
        case 4:
            return emit_mode::block;
        default:
            return emit_mode::cluster;
    }
}

} // namespace

// Reference: finalise_ctor_impl(), src/taylor_adaptive_batch.cpp:78-427.
tab_core::tab_core(sys_t sys, std::vector<double> state, std::uint32_t batch_size, config cfg)
    : m_impl(std::make_unique<impl>())
{
    auto &d = *m_impl;

    validate_ode_sys(sys);

    d.N = batch_size;
    d.high_accuracy = cfg.high_accuracy;
    d.compact_mode = cfg.compact_mode;
    d.device = cfg.device;
    d.emitter = cfg.emitter;
    d.cluster_kernel = cfg.cluster_kernel;
    d.exact_division = cfg.exact_division;
    d.sum_order = cfg.sum_order;
    if (d.sum_order < 0 || d.sum_order > 2) {
        throw std::invalid_argument("Invalid order of summation selected in an adaptive Taylor integrator in batch mode: "
                                    + std::to_string(d.sum_order) + " (0 automatic, 1 pairwise, 2 running sums)");
    }
    d.events_on_cluster = cfg.events_on_cluster;
    d.batch_semantics = cfg.batch_semantics;
    if (d.emitter < 0 || d.emitter > 4) {
        throw std::invalid_argument("Invalid code generator selected in an adaptive Taylor integrator in batch mode: "
                                    + std::to_string(d.emitter) + " (0 automatic, 1 unrolled, 2 cluster, 3 table, 4 block)");
    }
    if (d.cluster_kernel != 0 && d.cluster_kernel != 5 && d.cluster_kernel != 3 && d.cluster_kernel != 2
        && d.cluster_kernel != 1) {
        throw std::invalid_argument("Invalid wave-cluster generator selected in an adaptive Taylor integrator in batch mode: "
                                    + std::to_string(d.cluster_kernel) + " (0 automatic, or 5, 3, 2, 1)");
    }
    if (d.batch_semantics < 0 || d.batch_semantics > 3) {
        throw std::invalid_argument("Invalid batch semantics selected in an adaptive Taylor integrator in batch mode: "
                                    + std::to_string(d.batch_semantics) + " (0 reference, 1 lock-step loop, 2 per lane, 3 independent)");
    }
    // Developer overrides from the environment (experiments and the test matrix): they map onto the same fields.
    if (const char *m = std::getenv("HEYOKA_AMD_EMIT_MODE")) {
        const std::string ms(m);
        d.emitter = ms == "unrolled" ? 1 : (ms == "cluster" ? 2 : (ms == "table" ? 3 : (ms == "block" ? 4 : d.emitter)));
    }
    if (const char *ev = std::getenv("HEYOKA_AMD_ONE_LANE"); ev != nullptr && std::atoi(ev) == 0 && d.cluster_kernel == 0) {
        d.cluster_kernel = 3;
    }
    if (const char *ev = std::getenv("HEYOKA_AMD_PAIR_SPLIT"); ev != nullptr && std::atoi(ev) == 0
        && (d.cluster_kernel == 0 || d.cluster_kernel == 3)) {
        d.cluster_kernel = 2;
    }
    if (const char *ev = std::getenv("HEYOKA_AMD_EVENTS_ON_CLUSTER"); ev != nullptr && std::atoi(ev) == 0) {
        d.events_on_cluster = 1;
    }

    if (d.N == 0u) {
        throw std::invalid_argument("The batch size in an adaptive Taylor integrator cannot be zero");
    }

    if (state.size() % d.N != 0u) {
        throw std::invalid_argument("Invalid size detected in the initialization of an adaptive Taylor "
                                    "integrator: the state vector has a size of "
                                    + std::to_string(state.size()) + ", which is not a multiple of the batch size ("
                                    + std::to_string(d.N) + ")");
    }

    if (state.empty()) {
        state.resize(sys.size() * static_cast<std::size_t>(d.N));
    }

    if (state.size() / d.N != sys.size()) {
        throw std::invalid_argument("Inconsistent sizes detected in the initialization of an adaptive Taylor "
                                    "integrator: the state vector has a dimension of "
                                    + std::to_string(state.size() / d.N) + " and a batch size of "
                                    + std::to_string(d.N) + ", while the number of equations is "
                                    + std::to_string(sys.size()));
    }

    // Time.
    if (cfg.time.empty()) {
        d.time_hi.assign(d.N, 0.);
    } else if (cfg.time_is_scalar) {
        d.time_hi.assign(d.N, cfg.time[0]);
    } else {
        d.time_hi = std::move(cfg.time);
    }
    if (d.time_hi.size() != d.N) {
        throw std::invalid_argument("Invalid size detected in the initialization of an adaptive Taylor "
                                    "integrator: the time vector has a size of "
                                    + std::to_string(d.time_hi.size()) + ", which is not equal to the batch size ("
                                    + std::to_string(d.N) + ")");
    }
    d.time_lo.assign(d.N, 0.);

    if (cfg.tol && (!std::isfinite(*cfg.tol) || *cfg.tol < 0)) {
        throw std::invalid_argument("The tolerance in an adaptive Taylor integrator must be finite and positive, "
                                    "but it is "
                                    + fp_to_string(*cfg.tol) + " instead");
    }

    if (cfg.parallel_mode && !cfg.compact_mode) {
        throw std::invalid_argument("Parallel mode can be activated only in conjunction with compact mode");
    }

    d.tol = cfg.tol ? *cfg.tol : std::numeric_limits<double>::epsilon();
    d.dim = static_cast<std::uint32_t>(sys.size());
    d.state = std::move(state);

    // Decomposition + flattened program (with the event equations as extra functions, terminal events first,
    // reference: src/taylor_adaptive_batch.cpp:280-330).
    const detail::stopwatch sw_dc;
    d.tes = std::move(cfg.t_events);
    d.ntes = std::move(cfg.nt_events);
    if (d.has_events()) {
        for (const auto &ev : d.tes) {
            if (!std::isfinite(ev.cooldown)) {
                throw std::invalid_argument("Cannot set a non-finite cooldown value for a terminal event");
            }
        }
        for (const auto &ev : d.ntes) {
            if (!ev.callback) {
                throw std::invalid_argument("Cannot construct a non-terminal event with an empty callback");
            }
        }
        std::vector<expression> ev_eqs;
        for (const auto &ev : d.tes) {
            ev_eqs.push_back(ev.eq);
        }
        for (const auto &ev : d.ntes) {
            ev_eqs.push_back(ev.eq);
        }
        std::vector<std::uint32_t> ev_u;
        d.dc = taylor_decompose_sys(sys, ev_eqs, ev_u);
        d.prog = make_program(d.dc, d.dim);
        d.prog.ev_u = std::move(ev_u);
        d.te_cooldowns.assign(d.N, std::vector<std::optional<std::pair<double, double>>>(d.tes.size()));
    } else {
        d.dc = taylor_decompose_sys(sys);
        d.prog = make_program(d.dc, d.dim);
    }

    // (Stage log, in the reference's wording: src/taylor_01.cpp:439-440, :968.)
    detail::log_message(log_level::debug, "Taylor decomposition of " + std::to_string(d.dim) + " equations: " + std::to_string(d.dc.size())
                                              + " entries (" + std::to_string(d.prog.n_u) + " u variables, "
                                              + std::to_string(d.prog.nodes.size()) + " elementary functions)");
    detail::log_message(log_level::trace, "Taylor decomposition construction runtime: " + sw_dc.str());

    // Parameters.
    const auto tot_n_pars = d.prog.n_par;
    const auto pars_req = static_cast<std::size_t>(tot_n_pars) * d.N;
    if (cfg.pars.empty()) {
        cfg.pars.resize(pars_req);
    } else if (cfg.pars.size() != pars_req) {
        throw std::invalid_argument("Invalid number of parameter values passed to the constructor of an adaptive "
                                    "Taylor integrator in batch mode: "
                                    + std::to_string(cfg.pars.size())
                                    + " parameter value(s) were passed, but the ODE system contains "
                                    + std::to_string(tot_n_pars) + " parameter(s) (in batches of "
                                    + std::to_string(d.N) + ")");
    }
    d.pars = std::move(cfg.pars);

    d.order = taylor_order_from_tol(d.tol);

    // Index-range checks (the generated code indexes with 64-bit integers, but the public
    // interface shares the 32-bit batch size of the reference).
    if (static_cast<std::uint64_t>(d.dim) * (d.order + 1u) > std::numeric_limits<std::uint32_t>::max()) {
        throw std::overflow_error(
            "An overflow condition was detected in the computation of a jet of Taylor derivatives");
    }

    // Code generation + hiprtc compilation (works without a GPU).
    emit_options eo;
    eo.dev = dev_switches::from_env();
    eo.order = d.order;
    eo.high_accuracy = d.high_accuracy;
    eo.batch_size = d.N;
    eo.cluster_kernel = d.cluster_kernel;
    eo.exact_division = d.exact_division;
    eo.sum_order = d.sum_order;
    // NOTE: the stepper with events (mode 4) is implemented by the one-system-per-lane kernels: fully unrolled for
    // small decompositions, table-driven otherwise (HEYOKA_AMD_EMIT_MODE=table forces the latter).
    if (d.has_events()) {
        eo.mode = (d.prog.nodes.size() > 150u || choose_mode(d.emitter) == emit_mode::table) ? emit_mode::table
                                                                                            : emit_mode::unrolled;
        // Wave-cluster stepper for the system itself + the event equations from its jets, when both apply (event
        // equations which depend on a small part of the decomposition: distances, coordinates, angles, ...).
        // HEYOKA_AMD_EVENTS_ON_CLUSTER=0: always the one-system-per-lane steppers with events.
        if (choose_mode(d.emitter) == emit_mode::cluster && d.events_on_cluster == 0) {
            const auto prog0 = make_program(taylor_decompose_sys(sys), d.dim);
            auto eo2 = eo;
            eo2.mode = emit_mode::cluster;
            eo2.event_stepper = true;
            // The stepper may evaluate the event equations itself, take the final step size and update the state
            // (emit_options::ev_prog); lanes whose step is truncated at a terminal event are redone from the Taylor
            // coefficients afterwards.
            eo2.ev_prog = &d.prog;
            eo2.n_t_events = static_cast<std::uint32_t>(d.tes.size());
            auto m = emit_hip_module(prog0, eo2);
            std::string why;
            if (m.cluster_mode4) {
                auto eo_ev = eo;
                eo_ev.compact_tc = m.compact_tc;
                // (Event equations inside the stepper: the companion module only serves the compact Taylor coefficients.)
                auto evm = (m.events_in_stepper && m.compact_tc) ? emit_compact_tc_module(d.prog, eo_ev)
                                                                 : emit_event_jets(d.prog, eo_ev, why);
                if (!evm.source.empty()) {
                    d.cluster_events = true;
                    d.emitted = std::move(m);
                    d.emitted.notes += "; events: " + evm.notes;
                    d.ev_emitted = std::move(evm);
                    d.ev_cmod = hiprtc_compile(d.ev_emitted);
                }
            }
        }
    } else {
        eo.mode = choose_mode(d.emitter);
        // kw::compact_mode = true. In the reference it is a code-size / compile-time knob which also changes the order of
        // the additions inside the convolutions (running sums, src/math/prod.cpp:686-698, instead of products + pairwise
        // sum, :386-395) and costs little at run time. Here: the on-chip kernels stay whenever the planner can shape the
        // decomposition (their convolutions are FMA chains - running sums - already; code size does not grow with the
        // number of bodies); the straight-line generator adds in the compact order (sum_order = 2) and is kept only for
        // small decompositions; everything else runs on the rolled, table-driven steppers (one device function per
        // elementary function: the analogue of src/taylor_02.cpp:1194-1260). HEYOKA_AMD_EMIT_MODE / kw::emitter override.
        if (d.compact_mode && d.emitter == 0) {
            eo.unroll_max_nodes = 40;
        }
    }
    // (The order of the additions of compact mode, whatever generator is in charge - the staged table stepper deals the
    // terms of a convolution to several lanes otherwise.)
    if (d.compact_mode && eo.sum_order == 0) {
        eo.sum_order = 2;
    }
    const detail::stopwatch sw_gen;
    if (!d.cluster_events) {
        d.emitted = emit_hip_module(d.prog, eo);
    }
    // The planner's verdict: which generator, and - in its notes - why the others did not apply (the reasons of every
    // planner which was tried travel in emitted_module::notes; get_codegen_info() shows the same text).
    detail::log_message(log_level::info, "Taylor batch code generation: " + get_codegen_info());
    if (d.emitted.mode == emit_mode::table || d.emitted.cluster_fallback) {
        // A decomposition which left the on-chip steppers for a generic one is worth a line at the default level only
        // when it is big enough to matter.
        detail::log_message(d.prog.nodes.size() > 150u && !d.compact_mode && d.emitter == 0 ? log_level::warn : log_level::debug,
                            "the decomposition (" + std::to_string(d.prog.nodes.size())
                                + " elementary functions) runs on a generic stepper instead of a wave-cluster kernel: " + d.emitted.notes);
    }
    detail::log_message(log_level::trace, "Taylor batch code generation runtime: " + sw_gen.str());
    const detail::stopwatch sw_jit;
    d.cmod = hiprtc_compile(d.emitted);
    detail::log_message(log_level::trace, "Taylor batch hiprtc compilation runtime: " + sw_jit.str() + " ("
                                              + std::to_string(d.emitted.source.size()) + " bytes of HIP source)");

    for (const auto &ev : d.tes) {
        d.ev_has_rec = d.ev_has_rec || ev.recorder;
    }
    for (const auto &ev : d.ntes) {
        d.ev_has_rec = d.ev_has_rec || ev.recorder;
    }
    {
        // Terminal-event actions: checked against the system, one section each, the kernel in a module of its own.
        const auto svars = state_variables_of(sys);
        for (std::size_t e = 0; e < d.tes.size(); ++e) {
            if (d.tes[e].action) {
                d.act_sections.push_back(make_event_action_section(*d.tes[e].action, static_cast<std::uint32_t>(e), svars, d.prog.n_par));
            }
        }
        if (!d.act_sections.empty()) {
            d.act.source = make_event_action_source(d.act_sections);
            d.act.cm = hiprtc_compile_source(d.act.source);
        }
    }
    if (d.ev_has_rec) {
        // Recording callbacks: the kernels of the event log, in modules of their own.
        d.eo = eo;
        d.drow_cmod = hiprtc_compile_source(make_event_log_dout_source(d.prog, d.log_emit_options()));
        d.evr_cmod = hiprtc_compile_source(make_event_recorder_source(
            ed_max_detected(d.order, static_cast<std::uint32_t>(d.tes.size()), static_cast<std::uint32_t>(d.ntes.size()))));
    }

    d.eo = eo;
    d.sys = std::move(sys);
    d.last_h.assign(d.N, 0.);
    d.d_out.assign(static_cast<std::size_t>(d.dim) * d.N, 0.);
    d.step_res.assign(d.N, std::tuple{taylor_outcome::success, 0.});
    d.prop_res.assign(d.N, std::tuple{taylor_outcome::success, 0., 0., std::size_t(0)});
}

tab_core::tab_core() noexcept = default;

tab_core::tab_core(const tab_core &o) : m_impl(o.m_impl ? std::make_unique<impl>() : nullptr)
{
    if (!o.m_impl) {
        return;
    }
    const auto &s = *o.m_impl;
    // Bring the host mirrors of the source up to date, then deep-copy them. The compiled module
    // is shared (reference: shared_ptr<ta_jit_data>, include/heyoka/detail/i_data.hpp:125).
    s.to_host();
    s.fetch_step_res();
    s.fetch_prop_res();
    if (s.lasth_dev_newer) {
        s.d_lasth.download(s.last_h.data(), s.last_h.size() * sizeof(double), s.stream);
        s.lasth_dev_newer = false;
    }
    if (s.tc_dev_newer && s.dmod && s.d_tc.bytes() != 0u) {
        s.ensure_tc_expanded();
        s.tc.resize(static_cast<std::size_t>(s.dim) * (s.order + 1u) * s.N);
        s.d_tc.download(s.tc.data(), s.tc.size() * sizeof(double), s.stream);
        s.tc_dev_newer = false;
    }
    auto &d = *m_impl;
    d.sys = s.sys;
    d.dc = s.dc;
    d.prog = s.prog;
    d.order = s.order;
    d.tol = s.tol;
    d.high_accuracy = s.high_accuracy;
    d.compact_mode = s.compact_mode;
    d.emitter = s.emitter;
    d.cluster_kernel = s.cluster_kernel;
    d.exact_division = s.exact_division;
    d.sum_order = s.sum_order;
    d.events_on_cluster = s.events_on_cluster;
    d.batch_semantics = s.batch_semantics;
    d.N = s.N;
    d.dim = s.dim;
    d.device = s.device;
    d.emitted = s.emitted;
    d.eo = s.eo;
    d.cmod = s.cmod;
    d.cluster_events = s.cluster_events;
    d.ev_emitted = s.ev_emitted;
    d.ev_cmod = s.ev_cmod;
    // (The copy starts with an empty event log.)
    d.ev_has_rec = s.ev_has_rec;
    d.log_states = s.log_states;
    d.log_obs = s.log_obs;
    d.evr_cmod = s.evr_cmod;
    d.drow_cmod = s.drow_cmod;
    d.act_sections = s.act_sections;
    d.act.source = s.act.source;
    d.act.cm = s.act.cm;
    d.var = s.var;
    d.tstate = s.tstate;
    d.state = s.state;
    d.pars = s.pars;
    d.time_hi = s.time_hi;
    d.time_lo = s.time_lo;
    d.tc = s.tc;
    d.last_h = s.last_h;
    d.d_out = s.d_out;
    d.step_res = s.step_res;
    d.prop_res = s.prop_res;
    d.stream = s.stream;
    d.last_total_steps = s.last_total_steps;
    d.tes = s.tes;
    d.ntes = s.ntes;
    s.cooldowns_to_host();
    d.te_cooldowns = s.te_cooldowns;
    d.host_newer = true;
}

tab_core::tab_core(tab_core &&) noexcept = default;

tab_core &tab_core::operator=(const tab_core &o)
{
    if (this != &o) {
        *this = tab_core(o);
    }
    return *this;
}

tab_core &tab_core::operator=(tab_core &&) noexcept = default;

tab_core::~tab_core() = default;

const taylor_dc_t &tab_core::get_decomposition() const
{
    return m_impl->dc;
}
const taylor_program &tab_core::get_program() const
{
    return m_impl->prog;
}
std::uint32_t tab_core::get_batch_size() const
{
    return m_impl->N;
}
std::uint32_t tab_core::get_order() const
{
    return m_impl->order;
}
double tab_core::get_tol() const
{
    return m_impl->tol;
}
bool tab_core::get_high_accuracy() const
{
    return m_impl->high_accuracy;
}
std::uint64_t tab_core::get_event_detection_failures() const
{
    return m_impl->ed_failures;
}

bool tab_core::get_compact_mode() const
{
    return m_impl->compact_mode;
}
std::uint32_t tab_core::get_dim() const
{
    return m_impl->dim;
}
const tab_core::sys_t &tab_core::get_sys() const
{
    return m_impl->sys;
}
int tab_core::get_device() const
{
    return m_impl->device;
}
const std::vector<char> &tab_core::get_code_object() const
{
    return m_impl->cmod->code;
}

const std::string &tab_core::get_hip_source() const
{
    return m_impl->emitted.source;
}
const std::string &tab_core::get_internal_program() const
{
    return m_impl->emitted.internal_program;
}
std::string tab_core::get_codegen_info() const
{
    const auto &m = m_impl->emitted;
    const char *mode = m.mode == emit_mode::cluster
                           ? "cluster"
                           : (m.mode == emit_mode::table ? "table" : (m.mode == emit_mode::block ? "block" : "unrolled"));
    return std::string(mode) + " [lanes per system: " + std::to_string(m.lanes_per_system)
           + ", statements: " + std::to_string(m.n_statements) + "] " + m.notes;
}

double tab_core::get_compile_seconds() const
{
    return m_impl->cmod->compile_seconds;
}
std::uint64_t tab_core::get_scratch_per_wave() const
{
    return m_impl->emitted.scratch_per_wave;
}

const std::vector<double> &tab_core::get_time() const
{
    // (Polling the time after every step - benchmark/outer_ss_long_term_batch.cpp does - must not drag the state along.)
    m_impl->times_to_host();
    return m_impl->time_hi;
}

std::pair<const std::vector<double> &, const std::vector<double> &> tab_core::get_dtime() const
{
    m_impl->times_to_host();
    return {m_impl->time_hi, m_impl->time_lo};
}

void tab_core::set_time(const std::vector<double> &t)
{
    auto &d = *m_impl;
    if (t.size() != d.N) {
        throw std::invalid_argument("Invalid number of new times specified in a Taylor integrator in batch mode: the "
                                    "batch size is "
                                    + std::to_string(d.N) + ", but the number of specified times is "
                                    + std::to_string(t.size()));
    }
    d.to_host();
    d.time_hi = t;
    std::fill(d.time_lo.begin(), d.time_lo.end(), 0.);
    d.host_newer = true;
    ++d.time_gen;
}

void tab_core::set_time(double t)
{
    auto &d = *m_impl;
    d.to_host();
    std::fill(d.time_hi.begin(), d.time_hi.end(), t);
    std::fill(d.time_lo.begin(), d.time_lo.end(), 0.);
    d.host_newer = true;
    ++d.time_gen;
}

void tab_core::set_dtime(const std::vector<double> &hi, const std::vector<double> &lo)
{
    auto &d = *m_impl;
    if (hi.size() != d.N || lo.size() != d.N) {
        throw std::invalid_argument("Invalid number of new times specified in a Taylor integrator in batch mode: the "
                                    "batch size is "
                                    + std::to_string(d.N) + ", but the number of specified times is ("
                                    + std::to_string(hi.size()) + ", " + std::to_string(lo.size()) + ")");
    }
    // Checks on the values before anything is touched (dtime_checks(), include/heyoka/detail/taylor_common.hpp:232-249;
    // src/taylor_adaptive_batch.cpp:576-580).
    for (std::uint32_t i = 0; i < d.N; ++i) {
        if (!std::isfinite(hi[i]) || !std::isfinite(lo[i])) {
            throw std::invalid_argument("The components of the double-length representation of the time coordinate must "
                                        "both be finite, but they are "
                                        + fp_to_string(hi[i]) + " and " + fp_to_string(lo[i]) + " instead");
        }
        if (std::abs(hi[i]) < std::abs(lo[i])) {
            throw std::invalid_argument("The first component of the double-length representation of the time coordinate ("
                                        + fp_to_string(hi[i])
                                        + ") must not be smaller in magnitude than the second component ("
                                        + fp_to_string(lo[i]) + ")");
        }
    }
    d.to_host();
    for (std::uint32_t i = 0; i < d.N; ++i) {
        // Normalise (reference: normalise(), include/heyoka/detail/dfloat.hpp:125-139).
        const auto [u, v] = eft_add_dekker(hi[i], lo[i]);
        d.time_hi[i] = u;
        d.time_lo[i] = v;
    }
    d.host_newer = true;
    ++d.time_gen;
}

void tab_core::set_dtime(double hi, double lo)
{
    auto &d = *m_impl;
    set_dtime(std::vector<double>(d.N, hi), std::vector<double>(d.N, lo));
}

void tab_core::hold_host_refs() const
{
    m_impl->sticky_const_refs = true;
}

void tab_core::hold_time_refs() const
{
    m_impl->sticky_time_refs = true;
}

const std::vector<double> &tab_core::get_state() const
{
    m_impl->to_host();
    return m_impl->state;
}

double *tab_core::get_state_data()
{
    auto &d = *m_impl;
    d.to_host();
    d.host_newer = true;
    d.sticky_host_ptr = true;
    return d.state.data();
}

const std::vector<double> &tab_core::get_pars() const
{
    return m_impl->pars;
}

double *tab_core::get_pars_data()
{
    auto &d = *m_impl;
    d.to_host();
    d.host_newer = true;
    d.sticky_host_ptr = true;
    return d.pars.data();
}

void tab_core::set_state_values(const double *in)
{
    auto &d = *m_impl;
    d.to_host();
    std::copy(in, in + d.state.size(), d.state.begin());
    d.host_newer = true;
}

void tab_core::set_pars_values(const double *in)
{
    auto &d = *m_impl;
    d.to_host();
    std::copy(in, in + d.pars.size(), d.pars.begin());
    d.host_newer = true;
}

void tab_core::impl::ensure_tc_complete() const
{
    if (!tc_partial) {
        return;
    }
    tc_partial = false;
    tc_regenerated = true;
    ++tc_regens;
    auto &self = const_cast<impl &>(*this);
    auto a = self.base_args();
    a.state = evs_state.as<double>();
    a.time_hi = evs_thi.as<double>();
    a.time_lo = evs_tlo.as<double>();
    a.tc = d_tc.as<double>();
    // (The regeneration launch stores the Taylor coefficients and NOTHING else: the outputs of the step proper - event
    // jets, selector norms, max |x| - get null pointers, so that a generator regression faults instead of silently
    // rewriting them; the parameters are the ones the step ran with, snapshot below.)
    a.ev_tc = nullptr;
    a.max_abs_state = nullptr;
    a.sel_norms = nullptr;
    if (evs_pars.bytes() != 0u) {
        a.pars = evs_pars.as<double>();
    }
    a.mode = 4;
    a.pad = 3; // every workgroup stores its coefficients, nothing else is stored
    self.d_counters.zero(stream);
    dmod->launch_taylor(a);
    tc_expand_pending = emitted.compact_tc;
}

void tab_core::impl::ensure_tc_expanded() const
{
    ensure_tc_complete();
    if (!tc_expand_pending || !evj_mod) {
        return;
    }
    const doutc_kargs ea{d_tc.as<double>(), d_tc.as<double>(), nullptr, N, nullptr};
    evj_mod->launch("hy_tc_expand", N, 256, ea, stream);
    tc_expand_pending = false;
}

const std::vector<double> &tab_core::get_tc() const
{
    auto &d = *m_impl;
    d.check_tc_not_stale();
    d.ensure_tc_expanded();
    const auto sz = static_cast<std::size_t>(d.dim) * (d.order + 1u) * d.N;
    if (d.tc.size() != sz) {
        d.tc.assign(sz, 0.);
    }
    if (d.tc_dev_newer && d.dmod && d.d_tc.bytes() != 0u) {
        d.d_tc.download(d.tc.data(), sz * sizeof(double), d.stream);
        d.tc_dev_newer = false;
    }
    return d.tc;
}

const std::vector<double> &tab_core::get_last_h() const
{
    auto &d = *m_impl;
    if (d.lasth_dev_newer && d.dmod) {
        d.d_lasth.download(d.last_h.data(), d.last_h.size() * sizeof(double), d.stream);
        d.lasth_dev_newer = false;
    }
    return d.last_h;
}

const std::vector<double> &tab_core::get_d_output() const
{
    return m_impl->d_out;
}

// Reference: update_d_output(), src/taylor_adaptive_batch.cpp:2251-2327.
const std::vector<double> &tab_core::update_d_output(const std::vector<double> &t, bool rel_time)
{
    auto &d = *m_impl;
    if (t.size() != d.N) {
        throw std::invalid_argument("Invalid number of time coordinates specified for the dense output in a Taylor "
                                    "integrator in batch mode: the batch size is "
                                    + std::to_string(d.N) + ", but the number of time coordinates is "
                                    + std::to_string(t.size()));
    }
    d.ensure_device();
    d.ensure_tc();
    d.check_tc_not_stale();
    std::vector<double> hs(d.N);
    if (rel_time) {
        // Relative to the CURRENT time, i.e. to the end of the last step: h' = last_h + t (:2276-2280).
        const auto &lh = get_last_h();
        for (std::uint32_t i = 0; i < d.N; ++i) {
            hs[i] = lh[i] + t[i];
        }
    } else {
        d.times_to_host();
        const auto &lh = get_last_h();
        for (std::uint32_t i = 0; i < d.N; ++i) {
            // h' = t - (t_now - last_h), in double-length arithmetic.
            const auto t0 = dfloat(d.time_hi[i], d.time_lo[i]) - lh[i];
            hs[i] = static_cast<double>(dfloat(t[i]) - t0);
        }
    }
    if (d.d_dout.bytes() == 0u) {
        d.d_dout = device_buffer(d.d_out.size() * sizeof(double), d.device);
        d.d_douth = device_buffer(static_cast<std::size_t>(d.N) * sizeof(double), d.device);
    }
    d.d_douth.upload(hs.data(), hs.size() * sizeof(double), d.stream);
    d.ensure_tc_expanded();
    d.dmod->launch_dout(d.d_dout.as<double>(), d.d_tc.as<double>(), d.d_douth.as<double>(), d.N);
    d.d_dout.download(d.d_out.data(), d.d_out.size() * sizeof(double), d.stream);
    return d.d_out;
}

const std::vector<double> &tab_core::update_d_output(double t, bool rel_time)
{
    return update_d_output(std::vector<double>(m_impl->N, t), rel_time);
}

const std::vector<std::tuple<taylor_outcome, double>> &tab_core::get_step_res() const
{
    m_impl->fetch_step_res();
    return m_impl->step_res;
}

const std::vector<std::tuple<taylor_outcome, double, double, std::size_t>> &tab_core::get_propagate_res() const
{
    auto &d = *m_impl;
    d.fetch_prop_res();
    if (d.prop_res_override) {
        for (auto &r : d.prop_res) {
            std::get<0>(r) = *d.prop_res_override;
        }
        d.prop_res_override.reset();
        d.fix_step_limit = false;
    }
    return d.prop_res;
}

double *tab_core::device_state()
{
    m_impl->to_device();
    return m_impl->d_state.as<double>();
}
double *tab_core::device_pars()
{
    m_impl->to_device();
    return m_impl->d_pars.as<double>();
}
double *tab_core::device_time_hi()
{
    m_impl->to_device();
    return m_impl->d_thi.as<double>();
}
double *tab_core::device_time_lo()
{
    m_impl->to_device();
    return m_impl->d_tlo.as<double>();
}
double *tab_core::device_tc()
{
    m_impl->ensure_device();
    m_impl->ensure_tc();
    m_impl->ensure_tc_expanded();
    return m_impl->d_tc.as<double>();
}

void *tab_core::device_aux(int which)
{
    m_impl->ensure_device();
    switch (which) {
        case 0:
            return m_impl->d_nsteps.get();
        case 1:
            return m_impl->d_outcome.get();
        default:
            return m_impl->d_lasth.get();
    }
}

void tab_core::pack_results(double *dst)
{
    auto &d = *m_impl;
    d.to_device();
    const auto n = static_cast<std::size_t>(d.N), w = sizeof(double);
    // The results of the last propagation: on the device after a device-resident propagation (a step-limited batch first
    // gets the reference's batch-wide outcome, see fetch_prop_res()), otherwise uploaded from the host records.
    if (d.prop_res_dev_newer && (d.fix_step_limit || d.prop_res_override)) {
        d.fetch_prop_res();
    }
    if (d.prop_res_override) {
        // (A lock-step propagation which ended with step_limit / cb_stop: the batch-wide outcome get_propagate_res()
        // reports, src/taylor_adaptive_batch.cpp:1516.)
        for (auto &r : d.prop_res) {
            std::get<0>(r) = *d.prop_res_override;
        }
        d.prop_res_override.reset();
    }
    if (!d.prop_res_dev_newer) {
        std::vector<long long> oc(n);
        std::vector<double> mn(n), mx(n);
        std::vector<unsigned long long> ns(n);
        for (std::size_t i = 0; i < n; ++i) {
            const auto &[o, a, b, c] = d.prop_res[i];
            oc[i] = static_cast<long long>(o);
            mn[i] = a;
            mx[i] = b;
            ns[i] = static_cast<unsigned long long>(c);
        }
        d.d_outcome.upload(oc.data(), n * w, d.stream);
        d.d_minh.upload(mn.data(), n * w, d.stream);
        d.d_maxh.upload(mx.data(), n * w, d.stream);
        d.d_nsteps.upload(ns.data(), n * w, d.stream);
    }
    const auto cp = [&](std::size_t row, const void *src, std::size_t rows) {
        device_copy(dst + row * n, src, rows * n * w, d.device, d.stream);
    };
    cp(0, d.d_state.get(), d.dim);
    cp(d.dim, d.d_thi.get(), 1);
    cp(d.dim + 1u, d.d_tlo.get(), 1);
    cp(d.dim + 2u, d.d_outcome.get(), 1);
    cp(d.dim + 3u, d.d_nsteps.get(), 1);
    cp(d.dim + 4u, d.d_minh.get(), 1);
    cp(d.dim + 5u, d.d_maxh.get(), 1);
}

void tab_core::mark_device_modified()
{
    m_impl->to_device();
    m_impl->dev_newer = true;
    m_impl->times_fresh = false;
}

void tab_core::set_stream(void *s)
{
    m_impl->stream = s;
    if (m_impl->dmod) {
        m_impl->dmod->set_stream(s);
    }
}

void tab_core::set_device(int device)
{
    auto &d = *m_impl;
    if (device == d.device) {
        return;
    }
    // Bring everything back to the host, drop the device objects, switch.
    d.to_host();
    d.fetch_step_res();
    d.fetch_prop_res();
    d.cooldowns_to_host();
    (void)get_last_h();
    if (d.tc_dev_newer && d.dmod) {
        (void)get_tc();
    }
    d.dmod.reset();
    // (The rollback snapshot lives on the old device too; a pending step-limit fix-up / forced lock-step flag belonged to a
    // propagation which has been fetched above.)
    for (auto *b : {&d.d_state, &d.d_pars, &d.d_thi, &d.d_tlo, &d.d_lim, &d.d_tfhi, &d.d_tflo, &d.d_lasth, &d.d_outcome, &d.d_minh,
                    &d.d_maxh, &d.d_nsteps, &d.d_tc, &d.d_counters, &d.d_dout, &d.d_douth, &d.snap_state, &d.snap_thi, &d.snap_tlo}) {
        *b = {};
    }
    d.d_lim_src = nullptr;
    d.fix_step_limit = false;
    d.force_lockstep = false;
    // The auxiliary modules (event detection, post-step kernels of the lock-step loops) and the event buffers belong to
    // the old device as well: they are recreated on first use. A caller-provided stream belonged to the old device:
    // back to the default stream of the new one (set_stream() again if needed).
    d.ed_mod.reset();
    d.grid_mod.reset();
    d.evj_mod.reset();
    d.ar_mod.reset();
    d.tmap_mod.reset();
    d.d_tmap_in = {};
    d.d_tmap_out = {};
    d.d_ar_idx = {};
    d.ar_idx_dev.clear();
    for (auto &[k, v] : d.ar_variants) {
        (void)k;
        v.dm.reset();
    }
    if (d.log_rows != 0u && d.log_stash.empty()) {
        d.log_stash.resize(static_cast<std::size_t>(d.log_rows) * d.log_row_doubles());
        device_copy(d.log_stash.data(), d.d_ev_log.get(), d.log_stash.size() * sizeof(double), d.device, d.stream);
        stream_synchronize(d.device, d.stream);
    }
    d.evr_mod.reset();
    d.drow_mod.reset();
    d.obs_mod.reset();
    d.d_obs_stage = {};
    d.act.dm.reset();
    for (auto &[k, v] : d.sa_modules) {
        (void)k;
        v.dm.reset();
    }
    d.d_sa_cnt = {};
    for (auto &[k, v] : d.go_modules) {
        (void)k;
        v.dm.reset();
    }
    d.d_ev_log = {};
    d.d_evr_isrec = {};
    d.d_evr_lane = {};
    d.d_evr_blk = {};
    d.tc_expand_pending = false;
    d.tc_partial = false;
    for (auto *b : {&d.evs_state, &d.evs_pars, &d.evs_thi, &d.evs_tlo, &d.d_selnorms, &d.d_ev_cursor, &d.d_ev_rec, &d.d_ev_upd,
                    &d.d_ev_tc, &d.d_mas, &d.d_geps, &d.d_dirs, &d.d_cd_first, &d.d_cd_second, &d.d_cd_active, &d.d_ed_out,
                    &d.d_ed_counts, &d.d_ed_flags, &d.d_ed_wl, &d.d_te_stop, &d.d_retired}) {
        *b = {};
    }
    d.cd_host_newer = true;
    d.stream = nullptr;
    d.device = device;
    d.host_newer = true;
    d.dev_newer = false;
    d.tc_dev_newer = false;
    d.lasth_dev_newer = false;
}

void tab_core::synchronize()
{
    if (m_impl->dmod) {
        m_impl->dmod->synchronize();
    }
}

std::uint64_t tab_core::get_last_total_steps() const
{
    auto &d = *m_impl;
    d.fetch_prop_res();
    std::uint64_t tot = 0;
    for (const auto &r : d.prop_res) {
        tot += std::get<3>(r);
    }
    return tot;
}

std::vector<double> tab_core::get_kernel_ms_history(std::size_t n) const
{
    if (!m_impl->dmod) {
        return {};
    }
    return m_impl->dmod->kernel_ms_history(n);
}

void tab_core::raw_step(double *d_state, const double *d_pars, const double *d_time, double *d_h, double *d_tc,
                        std::uint64_t n_systems, void *d_tape)
{
    auto &d = *m_impl;
    d.ensure_device();
    // Scratch for the outputs the raw ABI does not expose.
    device_buffer tlo(n_systems * sizeof(double), d.device), oc(n_systems * sizeof(long long), d.device),
        lh(n_systems * sizeof(double), d.device);
    device_buffer tc_scratch;
    tlo.zero(d.stream);
    hy_kargs a{};
    a.state = d_state;
    a.pars = d_pars;
    // NOTE: mode 2 does not write the time back (the caller advances it, like step_impl() in the reference).
    a.time_hi = const_cast<double *>(d_time);
    a.time_lo = tlo.as<double>();
    a.lim = d_h;
    a.last_h = lh.as<double>();
    a.outcome = oc.as<long long>();
    d.d_counters.zero(d.stream);
    if (d_tc == nullptr && !d.is_cluster()) {
        tc_scratch = device_buffer(static_cast<std::size_t>(d.dim) * (d.order + 1u) * n_systems * sizeof(double),
                                   d.device);
        a.tc = tc_scratch.as<double>();
    } else {
        a.tc = d_tc;
    }
    a.N = n_systems;
    a.mode = 2;
    a.counters = d.d_counters.as<unsigned>();
    d.dmod->launch_taylor(a, d_tape);
    d.dmod->synchronize();
}

std::pair<std::size_t, std::size_t> tab_core::raw_tape_size_align(std::uint64_t n_systems)
{
    auto &d = *m_impl;
    d.ensure_device();
    // (0 bytes: this stepper keeps its Taylor coefficients on chip. 256: the alignment of a device allocation.)
    return {d.dmod->tape_bytes(n_systems), 256u};
}

void tab_core::raw_d_out_f(double *d_out, const double *d_tc, const double *d_h, std::uint64_t n_systems)
{
    auto &d = *m_impl;
    d.ensure_device();
    d.dmod->launch_dout(d_out, d_tc, d_h, n_systems);
    d.dmod->synchronize();
}

void tab_core::raw_step_e(double *d_jet, const double *d_state, const double *d_pars, const double *d_time, double *d_h,
                          double *d_max_abs_state, std::uint64_t n_systems, void *d_tape)
{
    auto &d = *m_impl;
    if (!with_events()) {
        throw std::invalid_argument("raw_step_e(): the stepper with events exists only in an integrator constructed with events");
    }
    d.ensure_device();
    d.ensure_event_buffers();
    const auto n = static_cast<std::size_t>(n_systems), w = sizeof(double);
    const auto tc_words = static_cast<std::size_t>(d.dim) * (d.order + 1u) * n;
    // Scratch for what the ABI does not expose. The stepper which evaluates the event equations itself also updates the
    // state it is given: it works on a copy (step_e leaves the state alone).
    device_buffer st(static_cast<std::size_t>(d.dim) * n * w, d.device), tlo(n * w, d.device), oc(n * sizeof(long long), d.device),
        lh(n * w, d.device), seln(3u * n * w, d.device), cnt(16u * sizeof(unsigned), d.device);
    device_copy(st.get(), d_state, st.bytes(), d.device, d.stream);
    tlo.zero(d.stream);
    cnt.zero(d.stream);
    hy_kargs a{};
    a.state = st.as<double>();
    a.pars = d_pars;
    a.time_hi = const_cast<double *>(d_time);
    a.time_lo = tlo.as<double>();
    a.lim = d_h;
    a.last_h = lh.as<double>();
    a.outcome = oc.as<long long>();
    a.tc = d_jet;
    a.ev_tc = d_jet + tc_words;
    a.max_abs_state = d_max_abs_state;
    a.sel_norms = seln.as<double>();
    a.N = n_systems;
    a.mode = 4;
    a.pad = 1; // the Taylor coefficients of every system
    a.counters = cnt.as<unsigned>();
    d.dmod->launch_taylor(a, d_tape);
    if (d.cluster_events && !d.evj_mod && d.ev_cmod) {
        d.evj_mod = std::make_unique<aux_module>(d.ev_cmod, d.device);
    }
    if (d.cluster_events && !d.emitted.events_in_stepper) {
        // (Jets of the event equations, extended norms and the step size from the jets of the state variables.)
        d.evj_mod->launch("hy_ev_jets", n_systems, 256, a, d.stream);
    }
    if (d.emitted.compact_tc && d.evj_mod) {
        // (The stepper left the rows of the variables defined by another state variable to be derived: x^[k] = v^[k-1] / k.)
        const doutc_kargs ea{d_jet, d_jet, nullptr, n_systems, nullptr};
        d.evj_mod->launch("hy_tc_expand", n_systems, 256, ea, d.stream);
    }
    // The step size which was taken.
    device_copy(d_h, lh.get(), n * w, d.device, d.stream);
    d.dmod->synchronize();
}

std::vector<double> make_vector_from(double x)
{
    return {x};
}

} // namespace heyoka_amd::detail
