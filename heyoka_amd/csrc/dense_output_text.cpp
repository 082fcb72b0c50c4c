// Dense output from the global buffer of Taylor coefficients. See dense_output_text.hpp.
#include "dense_output_text.hpp"
#include "hip_emit_detail.hpp"

#include <cassert>

namespace heyoka_amd
{
namespace emit_detail
{

bool defined_by_state_variable(const taylor_program &p, std::uint32_t i)
{
    return p.sv_defs[i].type == operand::kind::uvar && p.sv_defs[i].idx < p.n_eq;
}

compact_rows make_compact_rows(const taylor_program &p, const emit_options &opts)
{
    compact_rows ret;
    if (opts.compact_tc) {
        ret.parent.assign(p.n_eq, -1);
        ret.child.assign(p.n_eq, -1);
        for (std::uint32_t i = 0; i < p.n_eq; ++i) {
            if (defined_by_state_variable(p, i)) {
                ret.parent[i] = static_cast<int>(p.sv_defs[i].idx);
                ret.child[p.sv_defs[i].idx] = static_cast<int>(i);
            }
        }
    }
    return ret;
}

double rk_value(const emit_options &opts, std::uint32_t k)
{
    return opts.exact_division ? static_cast<double>(k) : 1. / static_cast<double>(k);
}

std::string derived_coeff_text(const emit_options &opts, const std::string &parent_coeff, const std::string &rk)
{
    return opts.exact_division ? ("(" + parent_coeff + " / " + rk + ")") : ("hy_mul_nc(" + parent_coeff + ", " + rk + ")");
}

void emit_compact_preamble(std::ostream &os, const emit_options &opts, const compact_rows *rows)
{
    // (An empty asm statement on the product: with -ffp-contract=fast the backend fuses whatever it can reach, pragmas or
    // not; a value which went through an asm operand is opaque to it.)
    os << "__device__ __forceinline__ double hy_mul_nc(double x, double y)\n{\n    double t = x * y;\n"
          "    asm(\"\" : \"+v\"(t));\n    return t;\n}\n";
    os << "__constant__ double hy_rk_c[" << (opts.order + 1u) << "] = {0.0";
    for (std::uint32_t k = 1; k <= opts.order; ++k) {
        os << "," << fp_literal(rk_value(opts, k));
    }
    os << "};\n";
    if (rows != nullptr) {
        const auto table = [&](const char *name, const std::vector<int> &t) {
            os << "__constant__ int " << name << "[" << t.size() << "] = {";
            for (const auto v : t) {
                os << v << ",";
            }
            os << "};\n";
        };
        table("hy_tc_parent", rows->parent);
        table("hy_tc_child", rows->child);
    }
}

namespace
{

// sum += term with the running compensation comp (reference: src/taylor_01.cpp:1074-1134):
// y = tmp - comp; t = sum + y; comp = (t - sum) - y; sum = t.
std::string compensated_step(const std::string &term, const std::string &sum, const std::string &comp)
{
    return "const double tmp = " + term + ";\nconst double y = tmp - " + comp + ";\nconst double t = " + sum + " + y;\n" + comp
           + " = (t - " + sum + ") - y;\n" + sum + " = t;\n";
}

} // namespace

void emit_plain_recurrence(std::ostream &os, const emit_options &opts)
{
    const auto order = opts.order;
    if (opts.high_accuracy) {
        os << "double res = c[0], comp = 0.0, cur_h = h;\n";
        os << "for (unsigned k = 1; k <= " << order << "u; ++k) {\n";
        os << compensated_step("c[(u64)k * N] * cur_h", "res", "comp") << "cur_h = cur_h * h;\n}\n";
    } else {
        os << "double res = c[(u64)" << order << "u * N];\n";
        os << "for (unsigned k = 1; k <= " << order << "u; ++k) {\n";
        os << "res = c[(u64)(" << order << "u - k) * N] + res * h;\n}\n";
    }
}

void emit_compact_recurrence(std::ostream &os, const emit_options &opts, bool want_v, const std::vector<std::string> &kids)
{
    const auto order = opts.order;
    const auto xk = derived_coeff_text(opts, "ck", "hy_rk_c[k + 1u]");
    if (opts.high_accuracy) {
        // (Ascending orders: res = c[0]; res += c[k] * h^k with the compensation of the plain recurrence.)
        os << "double ck = c[0];\ndouble cur_h = h;\n";
        if (want_v) {
            os << "double rv = ck, cv = 0.0;\n";
        }
        for (const auto &s : kids) {
            os << "double rx" << s << " = x0" << s << ", cx" << s << " = 0.0;\n";
        }
        os << "for (unsigned k = 0; k < " << order << "u; ++k) {\n";
        for (const auto &s : kids) {
            os << "{\n" << compensated_step(xk + " * cur_h", "rx" + s, "cx" + s) << "}\n";
        }
        os << "ck = c[(u64)(k + 1u) * N];\n";
        if (want_v) {
            os << "{\n" << compensated_step("ck * cur_h", "rv", "cv") << "}\n";
        }
        os << "cur_h = cur_h * h;\n}\n";
    } else {
        // (Descending orders: Horner from c[p] down, the first step of x without its addend.)
        os << "double ck = c[(u64)" << order << "u * N];\n";
        if (want_v) {
            os << "double rv = ck;\n";
        }
        for (const auto &s : kids) {
            os << "double rx" << s << " = 0.0;\n";
        }
        os << "for (unsigned k = " << order - 1u << "u;; --k) {\n";
        os << "ck = c[(u64)k * N];\n";
        if (want_v) {
            os << "rv = ck + rv * h;\n";
        }
        for (const auto &s : kids) {
            os << "rx" << s << " = (k == " << order - 1u << "u) ? " << xk << " : (" << xk << " + rx" << s << " * h);\n";
        }
        os << "if (k == 0u) break;\n}\n";
        for (const auto &s : kids) {
            os << "rx" << s << " = x0" << s << " + rx" << s << " * h;\n";
        }
    }
}

namespace
{

// The loops over the state variables of system s, up to where the results go. tc: the expression of the coefficient buffer.
std::string row_text(const emit_options &opts, const char *tc, const char *i)
{
    return std::string(tc) + " + ((u64)" + i + " * " + std::to_string(opts.order + 1u) + "u) * N + s";
}

// Full coefficients: one variable i per iteration, its value `res`.
void emit_plain_rows_loop(std::ostream &os, const taylor_program &p, const emit_options &opts, const char *tc, const char *store_res)
{
    os << "for (unsigned i = 0; i < " << p.n_eq << "u; ++i) {\n";
    os << "const double *c = " << row_text(opts, tc, "i") << ";\n";
    emit_plain_recurrence(os, opts);
    os << store_res << "}\n";
}

// Compact coefficients: one stored variable j per iteration, its value `rv` and - ch >= 0 - the value `rx` of the variable
// ch it defines.
void emit_compact_rows_loop(std::ostream &os, const taylor_program &p, const emit_options &opts, const char *tc, const char *store_rv,
                            const char *store_rx)
{
    os << "for (unsigned j = 0; j < " << p.n_eq << "u; ++j) {\n";
    os << "if (hy_tc_parent[j] >= 0) continue;\n";
    os << "const int ch = hy_tc_child[j];\n";
    os << "const double *c = " << row_text(opts, tc, "j") << ";\n";
    os << "const double x0 = (ch >= 0) ? " << tc << "[((u64)(unsigned)(ch < 0 ? 0 : ch) * " << (opts.order + 1u) << "u) * N + s] : 0.0;\n";
    emit_compact_recurrence(os, opts, true, {""});
    os << store_rv << "if (ch >= 0) " << store_rx << "}\n";
}

} // namespace

void emit_dout(std::ostringstream &os, const taylor_program &p, const emit_options &opts)
{
    os << "extern \"C\" __global__ void __launch_bounds__(256) hy_dout(" << detail::dout_kargs_parameters()
       << ")\n{\n";
    os << "const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;\nif (s >= N) return;\n";
    os << "const double h = hs[s];\n";
    emit_plain_rows_loop(os, p, opts, "tc", "out[(u64)i * N + s] = res;\n");
    os << "}\n";
}

std::string compact_tc_kernels_text(const taylor_program &p, const emit_options &opts)
{
    assert(opts.compact_tc);
    const auto n_eq = p.n_eq;
    const auto order = opts.order;
    const auto rows = make_compact_rows(p, opts);
    std::ostringstream os;
    emit_compact_preamble(os, opts, &rows);
    os << detail::doutc_kargs_text();
    // hy_dout_c: dense output (state update of a step with events) from the compact coefficients.
    os << "extern \"C\" __global__ void __launch_bounds__(256) hy_dout_c(const hy_doutc_args a)\n{\n";
    os << "const u64 N = a.N;\nconst u64 s = (u64)blockIdx.x * 256u + threadIdx.x;\nif (s >= N) return;\n";
    os << "const double h = a.hs[s];\n";
    os << "if (a.hfull != nullptr && h == a.hfull[s]) return;\n";
    emit_compact_rows_loop(os, p, opts, "a.tc", "a.out[(u64)j * N + s] = rv;\n", "a.out[(u64)(unsigned)ch * N + s] = rx;\n");
    os << "}\n";
    // hy_tc_expand: fills in the rows the stepper left out, for whoever reads the full array afterwards (get_tc(),
    // update_d_output(), continuous output, propagate_grid()).
    os << "extern \"C\" __global__ void __launch_bounds__(256) hy_tc_expand(const hy_doutc_args a)\n{\n";
    os << "const u64 N = a.N;\nconst u64 s = (u64)blockIdx.x * 256u + threadIdx.x;\nif (s >= N) return;\n";
    os << "double *tc = a.out;\n";
    os << "for (unsigned i = 0; i < " << n_eq << "u; ++i) {\n";
    os << "const int par = hy_tc_parent[i];\nif (par < 0) continue;\n";
    os << "double *c = tc + ((u64)i * " << (order + 1u) << "u) * N + s;\n";
    os << "const double *cp = tc + ((u64)(unsigned)par * " << (order + 1u) << "u) * N + s;\n";
    os << "for (unsigned k = 1; k <= " << order << "u; ++k) c[(u64)k * N] = "
       << derived_coeff_text(opts, "cp[(u64)(k - 1u) * N]", "hy_rk_c[k]") << ";\n}\n}\n";
    return os.str();
}

} // namespace emit_detail

emitted_module emit_compact_tc_module(const taylor_program &p, const emit_options &opts)
{
    emitted_module ret;
    ret.source = emit_detail::prelude() + emit_detail::compact_tc_kernels_text(p, opts);
    ret.kernel_name = "hy_dout_c";
    ret.block_size = 256;
    ret.lanes_per_system = 1;
    ret.mode = emit_mode::unrolled;
    ret.notes = std::to_string(p.ev_u.size()) + " event equation(s) evaluated by the stepper";
    return ret;
}

// One thread per row: the coefficient columns of the row's system are read at stride N - uncoalesced, but the rows are few
// against N * dim * (order + 1).
std::string make_event_log_dout_source(const taylor_program &p, const emit_options &opts)
{
    std::ostringstream os;
    os << emit_detail::prelude();
    os << detail::drow_kargs_text();
    if (opts.compact_tc) {
        const auto rows = emit_detail::make_compact_rows(p, opts);
        emit_detail::emit_compact_preamble(os, opts, &rows);
    }
    os << "extern \"C\" __global__ void __launch_bounds__(256) hy_dout_rows(const hy_drow_args a)\n{\n";
    os << "const u64 N = a.N;\nconst u64 r = (u64)blockIdx.x * 256u + threadIdx.x;\n";
    os << "u64 n = a.n_max;\nif (a.n_rows != nullptr && a.n_rows[0] < n) n = a.n_rows[0];\nif (r >= n) return;\n";
    os << "double *row = a.rows + r * a.row_doubles;\nconst u64 s = (u64)row[0];\nif (s >= N) return;\n";
    os << "double *out = row + 8;\n";
    // (Terminal event: the step was truncated at the event, the state after the step is the state at the event.)
    os << "if (row[1] == 0.0) {\nfor (unsigned i = 0; i < " << p.n_eq << "u; ++i) out[i] = a.state[(u64)i * N + s];\nreturn;\n}\n";
    os << "const double h = row[6];\n";
    if (opts.compact_tc) {
        emit_detail::emit_compact_rows_loop(os, p, opts, "a.tc", "out[j] = rv;\n", "out[(unsigned)ch] = rx;\n");
    } else {
        emit_detail::emit_plain_rows_loop(os, p, opts, "a.tc", "out[i] = res;\n");
    }
    os << "}\n";
    return os.str();
}

} // namespace heyoka_amd
