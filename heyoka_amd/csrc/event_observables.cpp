// Event-log observables. See event_observables.hpp.
#include "event_observables.hpp"

#include <algorithm>
#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cfunc.hpp"
#include "grid_observables.hpp"
#include "hip_emit_detail.hpp"
#include "kernel_args.hpp"

namespace heyoka_amd::detail
{

event_obs_section make_event_obs_section(const std::vector<expression> &obs, const std::vector<expression> &state_vars,
                                         std::uint32_t n_par)
{
    if (obs.empty()) {
        throw std::invalid_argument("The list of observables of the event log is empty");
    }
    const section_wording w{
        [](std::size_t o, const std::string &v) {
            return "The observable " + std::to_string(o) + " of the event log uses the variable '" + v
                   + "', which is not a state variable of the system";
        },
        [](std::uint32_t i, std::uint32_t n) {
            return "An observable of the event log uses par[" + std::to_string(i) + "], but the integrator has "
                   + std::to_string(n) + " parameter(s)";
        }};
    event_obs_section ret;
    static_cast<expr_section &>(ret) = make_expr_section(obs, state_vars, n_par, w);
    ret.n_obs = static_cast<std::uint32_t>(obs.size());
    ret.staged = ret.reads.size() > grid_obs_max_register_rows;
    if (const char *env = std::getenv("HEYOKA_AMD_EVENT_OBS")) {
        const std::string mode(env);
        if (mode == "registers") {
            ret.staged = false;
        } else if (mode == "staged") {
            ret.staged = true;
        } else if (!mode.empty()) {
            throw std::invalid_argument("Invalid value '" + mode + "' of HEYOKA_AMD_EVENT_OBS: 'registers' or 'staged'");
        }
    }
    return ret;
}

std::string make_event_log_obs_source(const taylor_program &p, const emit_options &opts, const event_obs_section &sec)
{
    const auto n_eq = p.n_eq;
    const auto order = opts.order;
    const auto &reads = sec.reads;
    const auto reads_row = [&](std::uint32_t i) { return std::binary_search(reads.begin(), reads.end(), i); };
    const auto rows = emit_detail::make_compact_rows(p, opts);
    // Where the sample of state row i lives: a named scalar, or the slot of the row of the log in the staging buffer.
    const auto slot = [&](std::uint32_t i) {
        const auto pos = static_cast<std::size_t>(std::lower_bound(reads.begin(), reads.end(), i) - reads.begin());
        return "(u64)" + std::to_string(pos) + "u * a.n_max";
    };
    const auto set = [&](std::uint32_t i, const std::string &value) {
        return (sec.staged ? "stg[" + slot(i) + "]" : "x" + std::to_string(i)) + " = " + value + ";\n";
    };
    const auto coeffs = [&](std::uint32_t i) {
        return "a.tc + ((u64)" + std::to_string(i) + "u * " + std::to_string(order + 1u) + "u) * N + s";
    };

    // (A compact row is sampled from the coefficients of the row which defines it: that row must hold coefficients of its
    // own. hy_dout_rows skips such a chain silently; an observable which reads it is refused.)
    for (const auto i : reads) {
        if (rows.derived(i) && rows.derived(p.sv_defs[i].idx)) {
            throw std::invalid_argument("An observable of the event log reads the state variable " + std::to_string(i)
                                        + ", which the compact Taylor coefficients define through another derived variable ("
                                        + std::to_string(p.sv_defs[i].idx) + "): this chain cannot be sampled");
        }
    }

    std::ostringstream os;
    os << emit_detail::prelude() << emit_detail::rules_source(sec.prog);
    os << drow_kargs_text();
    if (opts.compact_tc) {
        emit_detail::emit_compact_preamble(os, opts, nullptr);
    }
    // (hy_use(), see the section below. What it buys - the additions of the section contracted with the same products as in the
    // kernel of cfunc - is a property of the compiler, not of the language: the contract with cfunc is held by the GPU tests of
    // tests/test_event_observables_gpu.py, on both ways of holding the samples, and is only as strong as they are.)
    if (!sec.staged) {
        os << "__device__ __forceinline__ double hy_use(double x)\n{\n    asm volatile(\"\" : \"+v\"(x));\n    return x;\n}\n";
    }
    os << "// One thread per row of the log: the samples of the " << reads.size() << " state row(s) the observables read ("
       << (sec.staged ? "staged" : "registers") << "), then the observables.\n";
    os << "extern \"C\" __global__ void __launch_bounds__(256) hy_obs_rows(const hy_drow_args a)\n{\n";
    os << "const u64 N = a.N;\nconst u64 r = (u64)blockIdx.x * 256u + threadIdx.x;\n";
    os << "u64 n = a.n_max;\nif (a.n_rows != nullptr && a.n_rows[0] < n) n = a.n_rows[0];\nif (r >= n) return;\n";
    os << "double *row = a.rows + r * a.row_doubles;\nconst u64 s = (u64)row[0];\nif (s >= N) return;\n";
    if (sec.staged) {
        os << "double *stg = a.stage + r;\n";
    } else {
        for (const auto i : reads) {
            os << "double x" << i << ";\n";
        }
    }
    // (Terminal event: the step was truncated at the event, the state after the step is the state at the event.)
    os << "if (row[1] == 0.0) {\n";
    for (const auto i : reads) {
        os << set(i, "a.state[(u64)" + std::to_string(i) + "u * N + s]");
    }
    os << "} else {\nconst double h = row[6];\n(void)h;\n";
    if (opts.compact_tc) {
        for (std::uint32_t j = 0; j < n_eq; ++j) {
            if (rows.derived(j)) {
                continue;
            }
            // The rows defined by row j which are read: they are sampled from the coefficients of j and their own order 0.
            std::vector<std::uint32_t> kids;
            std::vector<std::string> sfx;
            for (const auto i : reads) {
                if (rows.parent[i] == static_cast<int>(j)) {
                    kids.push_back(i);
                    sfx.push_back("_" + std::to_string(i));
                }
            }
            const bool want_v = reads_row(j);
            if (!want_v && kids.empty()) {
                continue;
            }
            os << "{\nconst double *c = " << coeffs(j) << ";\n";
            for (const auto i : kids) {
                os << "const double x0_" << i << " = a.tc[((u64)" << i << "u * " << (order + 1u) << "u) * N + s];\n";
            }
            emit_detail::emit_compact_recurrence(os, opts, want_v, sfx);
            if (want_v) {
                os << set(j, "rv");
            }
            for (const auto i : kids) {
                os << set(i, "rx_" + std::to_string(i));
            }
            os << "}\n";
        }
    } else {
        for (const auto i : reads) {
            os << "{\nconst double *c = " << coeffs(i) << ";\n";
            emit_detail::emit_plain_recurrence(os, opts);
            os << set(i, "res") << "}\n";
        }
    }
    os << "}\n";
    // The section: the samples are read where they are used. Staged: through a volatile pointer - the loads are not replaced
    // by the values just stored, which would keep every sample alive in a register after all. Registers: through hy_use(), a
    // value of its own per use like a load of the compiled function - the compiler orders the operands of the additions, and
    // with them which product an addition is contracted with, by where their inputs are defined: samples which are all
    // defined ahead of the section round differently from cfunc in the last bit.
    const auto &sp = sec.prog;
    const auto code = emit_order0(sp, [&](std::uint32_t i) {
        return sec.staged ? "((const volatile double *)stg)[" + slot(i) + "]" : "hy_use(x" + std::to_string(i) + ")";
    });
    for (std::uint32_t k = 0; k < sp.n_par; ++k) {
        os << "const double par_" << k << " = a.pars[(u64)" << k << "u * N + s];\n";
    }
    if (sp.time_dependent) {
        os << "const double t_hi = row[4];\n";
    }
    os << code.body;
    // (Named results first: no store to the row ahead of a load from it.)
    for (std::size_t o = 0; o < code.outs.size(); ++o) {
        os << "const double r" << o << " = " << code.outs[o] << ";\n";
    }
    for (std::size_t o = 0; o < code.outs.size(); ++o) {
        os << "row[" << (8u + o) << "u] = r" << o << ";\n";
    }
    os << "}\n";
    return os.str();
}

} // namespace heyoka_amd::detail
