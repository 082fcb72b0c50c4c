// Taylor-map kernels of the variational integrators and the members of tab_core which use them. See taylor_map.hpp.
#include "taylor_map.hpp"

#include "tab_impl.hpp"

namespace heyoka_amd::detail
{

namespace
{

std::string hexf(double x)
{
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%a", x);
    return buf;
}

} // namespace

std::uint32_t taylor_map_schedule::row(std::uint32_t i, std::uint32_t t) const
{
    std::uint32_t k = 0;
    while (k + 1u < first_term.size() && t >= first_term[k + 1u]) {
        ++k;
    }
    return row_base[k] + i * count[k] + (t - first_term[k]);
}

taylor_map_schedule make_taylor_map_schedule(std::uint32_t n_orig, std::uint32_t n_args, std::uint32_t order)
{
    if (n_orig == 0u || n_args == 0u || order == 0u) {
        throw std::invalid_argument("A Taylor map needs at least one state variable, one argument and order one");
    }
    taylor_map_schedule s;
    s.n_orig = n_orig;
    s.n_args = n_args;
    s.order = order;
    std::map<std::vector<std::uint32_t>, std::uint32_t> pos;
    std::uint32_t row = 0;
    for (std::uint32_t k = 0; k <= order; ++k) {
        // (The enumeration of var_ode_sys: the rows of the state are numbered with it.)
        auto alphas = heyoka_amd::detail::multi_indices_of_order(n_args, k);
        s.first_term.push_back(s.n_terms());
        s.count.push_back(static_cast<std::uint32_t>(alphas.size()));
        s.row_base.push_back(row);
        row += n_orig * static_cast<std::uint32_t>(alphas.size());
        for (auto &a : alphas) {
            double fact = 1;
            for (const auto e : a) {
                for (std::uint32_t q = 2; q <= e; ++q) {
                    fact *= q;
                }
            }
            std::uint32_t par = 0, last = 0;
            if (k != 0u) {
                last = n_args - 1u;
                while (a[last] == 0u) {
                    --last;
                }
                auto b = a;
                --b[last];
                par = pos.at(b);
            }
            pos.emplace(a, s.n_terms());
            s.parent.push_back(par);
            s.last.push_back(last);
            s.rfact.push_back(1. / fact);
            s.alpha.push_back(std::move(a));
        }
    }
    return s;
}

std::size_t taylor_map_lds_bytes()
{
    if (const char *ev = std::getenv("HEYOKA_AMD_TMAP_LDS_BYTES")) {
        const auto v = std::atoll(ev);
        if (v > 0) {
            return static_cast<std::size_t>(v);
        }
    }
    return taylor_map_default_lds_bytes;
}

namespace
{

// The terms of the outputs [i0, i1): every monomial right before the accumulations which use it. coef(i, t): the text of
// the pre-scaled coefficient s_{i, alpha_t} * RN(1 / alpha_t!).
template <typename Coef>
void emit_terms(std::ostringstream &o, const taylor_map_schedule &s, std::uint32_t i0, std::uint32_t i1, const char *ind,
                const Coef &coef)
{
    for (auto i = i0; i < i1; ++i) {
        o << ind << "double o" << i << " = " << coef(i, 0u) << ";\n";
    }
    for (std::uint32_t t = 1; t < s.n_terms(); ++t) {
        o << ind << "const double m" << t << " = ";
        if (s.parent[t] == 0u) {
            o << "d" << s.last[t];
        } else {
            o << "m" << s.parent[t] << " * d" << s.last[t];
        }
        o << ";\n";
        for (auto i = i0; i < i1; ++i) {
            o << ind << "o" << i << " = __builtin_fma(" << coef(i, t) << ", m" << t << ", o" << i << ");\n";
        }
    }
}

} // namespace

std::string make_taylor_map_source(std::uint32_t n_orig, std::uint32_t n_args, std::uint32_t order, std::size_t lds_bytes,
                                   std::string *note)
{
    const auto s = make_taylor_map_schedule(n_orig, n_args, order);
    const auto nt = s.n_terms();

    // Outputs per group of the cloud kernel.
    const auto per_output = static_cast<std::size_t>(nt) * sizeof(double);
    if (per_output > taylor_map_max_static_lds_bytes) {
        // (A group holds at least one output: beyond this the array of the cloud kernel could not be declared - and the
        // straight-line code of n_orig * n_terms fma would take hiprtc minutes. The terms are not chunked.)
        throw not_implemented_error("The Taylor map of a variational system with " + std::to_string(n_args) + " arguments at order "
                                    + std::to_string(order) + " is not available: the " + std::to_string(nt)
                                    + " coefficients of a single output (" + std::to_string(per_output)
                                    + " bytes) exceed the " + std::to_string(taylor_map_max_static_lds_bytes)
                                    + " bytes of LDS a workgroup can declare");
    }
    auto gsz = static_cast<std::uint32_t>(std::min<std::size_t>(n_orig, std::max<std::size_t>(1, lds_bytes / per_output)));
    const auto n_groups = (n_orig + gsz - 1u) / gsz;
    {
        std::ostringstream msg;
        msg << "taylor map (" << n_orig << ", " << n_args << ", " << order << "): " << nt << " terms per output, "
            << static_cast<std::size_t>(n_orig) * per_output << " bytes of coefficients per system; hy_tmap_cloud: ";
        if (n_groups == 1u) {
            msg << "all outputs in one pass";
        } else {
            msg << "grouped outputs: the coefficients of a system exceed the " << lds_bytes
                << " bytes of LDS allowed per workgroup, " << n_groups << " passes of at most " << gsz << " outputs ("
                << gsz * per_output << " bytes each)";
        }
        if (note != nullptr) {
            *note = msg.str();
        }
    }

    std::ostringstream o;
    o << "// Taylor map: n_orig_sv = " << n_orig << ", n_args = " << n_args << ", order = " << order << ", " << nt
      << " terms per output.\n";
    o << tmap_kargs_text() << tmap_cloud_kargs_text() << R"HIP(
extern "C" __global__ void __launch_bounds__(256) hy_tmap(const hy_tmap_args a)
{
    const unsigned long long sys = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (sys >= a.N) return;
    const unsigned long long N = a.N;
    const double *st = a.state + sys;
)HIP";
    for (std::uint32_t j = 0; j < n_args; ++j) {
        o << "    const double d" << j << " = a.in[" << j << "ull * N + sys];\n";
    }
    emit_terms(o, s, 0, n_orig, "    ", [&](std::uint32_t i, std::uint32_t t) {
        std::string c = "st[" + std::to_string(s.row(i, t)) + "ull * N]";
        if (s.rfact[t] != 1.) {
            c = "(" + c + " * " + hexf(s.rfact[t]) + ")";
        }
        return c;
    });
    for (std::uint32_t i = 0; i < n_orig; ++i) {
        o << "    a.out[" << i << "ull * N + sys] = o" << i << ";\n";
    }
    o << "}\n\n";

    // The cloud kernel. (The table of the reciprocal factorials serves the staging pass only: the loop over the samples reads
    // pre-scaled coefficients.)
    o << "static __device__ const double hy_tmap_rf[" << nt << "] = {";
    for (std::uint32_t t = 0; t < nt; ++t) {
        o << (t == 0u ? "" : ", ") << hexf(s.rfact[t]);
    }
    o << "};\n\n";
    o << "extern \"C\" __global__ void __launch_bounds__(256) hy_tmap_cloud(const hy_tmap_cloud_args a)\n{\n";
    o << "    __shared__ double cf[" << static_cast<std::size_t>(gsz) * nt << "];\n";
    o << R"HIP(    const unsigned long long sys = blockIdx.x / a.blocks_per_sys;
    const unsigned blk = blockIdx.x - (unsigned)sys * a.blocks_per_sys;
    if (sys >= a.N) return;
    const unsigned long long N = a.N, ns = a.n_samples;
    const unsigned long long stride = 256ull * a.blocks_per_sys;
    const double *dl = a.delta + (a.shared ? 0ull : sys * )HIP"
      << n_args << R"HIP(ull * ns);
    double *op = a.out + sys * )HIP"
      << n_orig << "ull * ns;\n";
    for (std::uint32_t g = 0; g < n_groups; ++g) {
        const auto i0 = g * gsz, i1 = std::min(n_orig, i0 + gsz), gn = i1 - i0;
        o << "    // Outputs [" << i0 << ", " << i1 << "): coefficients cf[t * " << gn << " + (i - " << i0 << ")].\n";
        if (g != 0u) {
            o << "    __syncthreads();\n";
        }
        o << "    for (unsigned q = threadIdx.x; q < " << gn * nt << "u; q += 256u) {\n";
        o << "        const unsigned t = q / " << gn << "u, i = " << i0 << "u + (q - t * " << gn << "u);\n";
        o << "        unsigned row = i;\n";
        for (std::uint32_t k = 1; k <= order; ++k) {
            o << "        if (t >= " << s.first_term[k] << "u) row = " << s.row_base[k] << "u + i * " << s.count[k] << "u + (t - "
              << s.first_term[k] << "u);\n";
        }
        o << "        cf[q] = a.state[(unsigned long long)row * N + sys] * hy_tmap_rf[t];\n";
        o << "    }\n";
        o << "    __syncthreads();\n";
        o << "    for (unsigned long long m = 256ull * blk + threadIdx.x; m < ns; m += stride) {\n";
        // (A compiler-only fence: without it the loop-invariant coefficient reads are hoisted out of the loop into
        // registers - all n_orig * n_terms of them, 372 VGPRs at (6, 6, 2) and scratch at (6, 6, 3) - instead of being
        // broadcast from LDS where they are used. It emits no instruction.)
        o << "        __atomic_signal_fence(__ATOMIC_SEQ_CST);\n";
        for (std::uint32_t j = 0; j < n_args; ++j) {
            o << "        const double d" << j << " = dl[" << j << "ull * ns + m];\n";
        }
        emit_terms(o, s, i0, i1, "        ", [&](std::uint32_t i, std::uint32_t t) {
            return "cf[" + std::to_string(t * gn + (i - i0)) + "]";
        });
        for (auto i = i0; i < i1; ++i) {
            o << "        op[" << i << "ull * ns + m] = o" << i << ";\n";
        }
        o << "    }\n";
    }
    o << "}\n";
    return o.str();
}

// ---- tab_core: variational integrators ----

namespace
{

// The state a variational integrator starts from (reference: finalise_ctor_impl(), src/taylor_adaptive_batch.cpp:177-217,
// and setup_variational_ics_varpar(), src/detail/setup_variational_ics.cpp:49-121): a state of n_orig_sv * batch_size
// values (or none) is extended with the initial conditions of the variational variables - 1 where a first-order derivative
// is taken with respect to its own state variable, 0 elsewhere. Anything the generic constructor rejects with a message of
// its own (batch size zero, a size which is not a multiple of it) is passed through.
std::vector<double> variational_state(const var_ode_sys &vsys, std::vector<double> state, std::uint32_t batch_size)
{
    if (!vsys.is_valid()) {
        throw std::invalid_argument("Cannot construct an integrator from a default-constructed var_ode_sys");
    }
    if (batch_size == 0u || state.size() % batch_size != 0u) {
        return state;
    }
    const auto &sys = vsys.get_sys();
    const std::size_t n_orig = vsys.get_n_orig_sv(), bs = batch_size;
    if (state.empty()) {
        state.resize(n_orig * bs);
    }
    if (state.size() / bs == sys.size()) {
        return state;
    }
    if (state.size() / bs != n_orig) {
        throw std::invalid_argument(
            "Inconsistent sizes detected in the initialization of a variational adaptive Taylor "
            "integrator in batch mode: the state vector has a dimension of "
            + std::to_string(state.size()) + " (in batches of " + std::to_string(bs)
            + "), while the "
              "total number of equations is "
            + std::to_string(sys.size())
            + ". The size of the state vector must be "
              "equal either to the total number of equations times the batch size, or to the number of original "
              "(i.e., non-variational) equations, which for this system is "
            + std::to_string(n_orig) + ", times the batch size");
    }
    state.resize(sys.size() * bs);
    const auto &vargs = vsys.get_vargs();
    const auto &didx = vsys.get_didx();
    for (auto e = n_orig; e < sys.size(); ++e) {
        const auto &[comp, alpha] = didx[e];
        std::uint32_t total = 0;
        std::size_t which = 0;
        for (std::size_t j = 0; j < alpha.size(); ++j) {
            total += alpha[j];
            if (alpha[j] != 0u) {
                which = j;
            }
        }
        if (total == 1u && vargs[which] == sys[comp].first) {
            std::fill(state.begin() + static_cast<std::ptrdiff_t>(e * bs), state.begin() + static_cast<std::ptrdiff_t>((e + 1u) * bs), 1.);
        }
    }
    return state;
}

} // namespace

tab_core::tab_core(const var_ode_sys &vsys, std::vector<double> state, std::uint32_t batch_size, config cfg)
    : tab_core(vsys.is_valid() ? vsys.get_sys() : sys_t{}, variational_state(vsys, std::move(state), batch_size), batch_size,
               std::move(cfg))
{
    auto &d = *m_impl;
    auto v = std::make_shared<impl::var_data>();
    v->vsys = vsys;
    const auto n_args = static_cast<std::uint32_t>(vsys.get_vargs().size());
    if (n_args != 0u) {
        // The module of the map is generated and compiled with the integrator (like the module of the event actions) and
        // loaded at the first evaluation.
        const detail::stopwatch sw;
        std::string note;
        // (The kernels address the state rows by the closed-form layout of the schedule: every row must be the equation of
        // vsys with that component and multi-index.)
        const auto sch = make_taylor_map_schedule(vsys.get_n_orig_sv(), n_args, vsys.get_order());
        const auto &didx = vsys.get_didx();
        bool same = sch.dim() == d.dim && didx.size() == d.dim;
        for (std::uint32_t i = 0; same && i < sch.n_orig; ++i) {
            for (std::uint32_t t = 0; same && t < sch.n_terms(); ++t) {
                const auto &e = didx[sch.row(i, t)];
                same = e.first == i && e.second == sch.alpha[t];
            }
        }
        if (!same) {
            throw std::runtime_error("Internal error: the Taylor-map schedule does not match the variational system");
        }
        try {
            v->tmap_source = make_taylor_map_source(sch.n_orig, n_args, sch.order, taylor_map_lds_bytes(), &note);
            detail::log_message(log_level::info, note);
            v->tmap_cmod = hiprtc_compile_source(v->tmap_source);
            detail::log_message(log_level::trace, "taylor map: module generation + compilation runtime: " + sw.str());
        } catch (const not_implemented_error &e) {
            // A map too large for the kernels: the integrator itself is fine, the evaluations of the map say why they cannot run.
            v->tmap_why = e.what();
            detail::log_message(log_level::warn, v->tmap_why);
        }
    } else {
        v->tmap_why = "This variational integrator has no variational arguments: there is no Taylor map";
    }
    d.var = std::move(v);
    d.tstate.assign(static_cast<std::size_t>(vsys.get_n_orig_sv()) * d.N, 0.);
}

bool tab_core::is_variational() const noexcept
{
    return m_impl && m_impl->var;
}

namespace
{

void check_variational(const tab_core &c, const char *fname)
{
    if (!c.is_variational()) {
        throw std::invalid_argument(std::string("The function '") + fname
                                    + "()' cannot be invoked on non-variational batch integrators");
    }
}

} // namespace

std::uint32_t tab_core::get_n_orig_sv() const noexcept
{
    return is_variational() ? m_impl->var->vsys.get_n_orig_sv() : m_impl->dim;
}

const var_ode_sys &tab_core::get_vsys(const char *fname) const
{
    check_variational(*this, fname);
    return m_impl->var->vsys;
}

const std::vector<double> &tab_core::get_tstate() const
{
    check_variational(*this, "get_tstate");
    return m_impl->tstate;
}

tab_core::module_view tab_core::taylor_map_module() const
{
    check_variational(*this, "taylor_map_source");
    if (!m_impl->var->tmap_cmod) {
        throw not_implemented_error(m_impl->var->tmap_why);
    }
    return {m_impl->var->tmap_source, m_impl->var->tmap_cmod->code};
}

void tab_core::eval_taylor_map_device(const double *d_in, double *d_out)
{
    check_variational(*this, "eval_taylor_map_device");
    auto &d = *m_impl;
    if (!d.var->tmap_cmod) {
        throw not_implemented_error(m_impl->var->tmap_why);
    }
    d.before_kernel();
    if (!d.tmap_mod) {
        d.tmap_mod = std::make_unique<aux_module>(d.var->tmap_cmod, d.device);
    }
    const tmap_kargs ka{d.d_state.as<double>(), d_in, d_out, d.N};
    d.tmap_mod->launch("hy_tmap", d.N, 256, ka, d.stream);
}

const std::vector<double> &tab_core::eval_taylor_map(const double *in, std::size_t n)
{
    check_variational(*this, "eval_taylor_map");
    auto &d = *m_impl;
    const std::size_t bs = d.N, nvargs = d.var->vsys.get_vargs().size();
    if (n % bs != 0u) {
        throw std::invalid_argument("Unable to compute the Taylor map: the input range of values has a "
                                    "size of "
                                    + std::to_string(n) + ", which is not a multiple of the batch size " + std::to_string(bs));
    }
    if (n / bs != nvargs) {
        throw std::invalid_argument("Unable to compute the Taylor map: the input range of values has a "
                                    "size of "
                                    + std::to_string(n / bs) + " (in batches of " + std::to_string(bs)
                                    + "), but the number of variational arguments is " + std::to_string(nvargs));
    }
    if (nvargs == 0u) {
        // (Nothing to expand in: the map is the state itself.)
        const auto &st = get_state();
        d.tstate.assign(st.begin(), st.begin() + static_cast<std::ptrdiff_t>(d.tstate.size()));
        return d.tstate;
    }
    d.ensure_device();
    if (d.d_tmap_in.bytes() != n * sizeof(double)) {
        d.d_tmap_in = device_buffer(n * sizeof(double), d.device);
        d.d_tmap_out = device_buffer(d.tstate.size() * sizeof(double), d.device);
    }
    d.d_tmap_in.upload(in, n * sizeof(double), d.stream);
    eval_taylor_map_device(d.d_tmap_in.as<double>(), d.d_tmap_out.as<double>());
    d.d_tmap_out.download(d.tstate.data(), d.tstate.size() * sizeof(double), d.stream);
    return d.tstate;
}

void tab_core::eval_taylor_map_cloud(const double *d_delta, double *d_out, std::uint64_t n_samples, bool shared)
{
    check_variational(*this, "eval_taylor_map_cloud");
    auto &d = *m_impl;
    if (!d.var->tmap_cmod) {
        throw not_implemented_error(m_impl->var->tmap_why);
    }
    if (n_samples == 0u) {
        return;
    }
    d.before_kernel();
    if (!d.tmap_mod) {
        d.tmap_mod = std::make_unique<aux_module>(d.var->tmap_cmod, d.device);
    }
    // Workgroups per system: every block of 256 samples its own workgroup until the grid holds a few workgroups per CU
    // slot; beyond that a workgroup strides over several blocks of samples and its staging pass is amortised over them.
    const std::uint64_t chunks = (n_samples + 255u) / 256u, target = 8192;
    const auto bps = static_cast<unsigned>(std::min<std::uint64_t>(chunks, std::max<std::uint64_t>(1, (target + d.N - 1u) / d.N)));
    const tmap_cloud_kargs ka{d.d_state.as<double>(), d_delta, d_out, d.N, n_samples, bps, shared ? 1u : 0u};
    d.tmap_mod->launch("hy_tmap_cloud", static_cast<std::uint64_t>(d.N) * bps * 256u, 256, ka, d.stream);
}

} // namespace heyoka_amd::detail
