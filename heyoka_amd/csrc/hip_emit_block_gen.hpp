// The generator of the block-mode kernel (one ODE system per workgroup, see hip_emit_block.cpp): one object per call of
// emit_block(), its stages in the order the text is produced. Private to hip_emit_block*.cpp:
//   hip_emit_block.cpp       emit_block() (the driver), the switches, plan() and the geometry, input_jets(), base_tables(),
//                            pair_phase_applicable(), the generic cluster phase generic_body(), module_text(), result()
//   hip_emit_block_pair.cpp  the pair phase ("v2 cluster phase": point-mass pair clusters, rolled order loop):
//                            pair_parameters(), pair_descriptors(), pair_merged_glue(), pair_fused_last_level(),
//                            pair_lds_mirrors(), pair_order0(), pair_glue_levels(), pair_recursion(), pair_order_loop()
// The data the stages share is grouped in the structs below; a stage reads what the stages before it left there.
#pragma once

#include <map>
#include <optional>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "hip_emit_cluster_plan.hpp"
#include "hip_emit_detail.hpp"

namespace heyoka_amd::block_detail
{

using cluster_detail::cluster_plan;
using cluster_detail::is_var;
using cluster_detail::pair_pattern;
using emit_detail::ssa_emitter;

// ---- HEYOKA_AMD_BLOCK_OPTS (emit_options::dev.block_opts), parsed once at the top of emit_block(). ----
// A list of items separated by ',' or ':'; an item is `name` (value 1) or `name=INT`; the first occurrence of a name wins,
// unknown names are ignored. The A/B harness of the block-mode kernel (profiles/experiments/): every item switches ONE
// ingredient, the comments where a switch is read say what was measured with it. THE list of the switches:
//   bs=N        workgroup size in lanes (default: 128 up to 128 clusters, 256, 512 for the pair phase beyond 1024 clusters)
//   nopad       no slot of padding between the output blocks of the slab
//   perm        clusters dealt into groups of 32 whose LDS reads of the input jets are free of bank conflicts
//   licm        machine-level loop-invariant code motion left on for the pair phase (changes the compile flags only)
//   M=N         pair phase: rows (orders) of the two tape members kept in registers for the whole step
//   G=N         ... rounds per pipeline group
//   D=N         ... depth of the tape-load pipeline, in slots
//   hand=N      ... most recent rows handed over from order to order in registers
//   reg_high    ... the high member of a slot selected from the rows in registers (=2: behind a wave-uniform branch)
//   hoist       ... cluster descriptors loaded once per step (=0: at the head of every group)
//   keepdz      ... order-0 differences of the clusters kept in registers through the orders (=0: re-read)
//   nopp        ... no ping-pong of the LDS operands: one register set (=0: two sets)
//   div         ... quotients as divisions instead of products with reciprocals + one correction
//   split       ... the two tape members in separate halves of the tape instead of interleaved
//   xpf         ... cross-group prefetch of the high rows of the first slots
//   unpacked    glue: one index table per operand position instead of packed records
//   noglueperm  glue: nodes of a merged level on the lanes in the order of the decomposition
//   nofuse      glue: the last level as a phase of its own, not fused into the state recursion
//   dbuf        glue: state-variable slots double-buffered by the parity of the order
//   exp=N       timing experiments, WRONG results: 1 = no slots beyond slot 0, 2 = no glue arithmetic, 3 = no LDS reads
//               in the slots, 4 = no tape loads in the slots, 34 = both, 5 = glue operands from conflict-free addresses
// A switch whose default depends on the geometry is "not given" (empty) until the stage which resolves it.
struct block_switches {
    using opt = std::optional<int>;
    opt bs;
    bool nopad = false, perm = false, licm = false;
    opt M, G, D, hand, hoist, keepdz, nopp;
    int reg_high = 0;
    int div = 0, split = 0, xpf = 0;
    int unpacked = 0, noglueperm = 0, nofuse = 0, dbuf = 0;
    int exp = 0;
    static block_switches parse(const std::string &list);
};

// ---- Plan and geometry of the workgroup (plan(); the pair pattern and the final bs: pair_phase_applicable()). ----
struct block_geometry {
    cluster_plan pl;
    pair_pattern pp;
    // bs: lanes per workgroup. NOTE: final only after pair_phase_applicable() (the pair phase runs large systems on 512
    // lanes); no stage before it reads bs, and n_iter / sv_rounds are set together with it.
    std::uint32_t nc = 0, ncp = 0, bs = 0, n_ext = 0, n_out = 0, n_cst = 0, n_sto = 0, n_slots = 0;
    std::uint32_t n_iter = 0;    // rounds of the cluster phase: clusters per lane
    std::uint32_t sv_rounds = 0; // state variables per lane
    bool wide = false;           // slots do not fit 16 bits
    const std::vector<std::uint32_t> &t0() const { return pl.clusters[0]; } // the template cluster
    void set_workgroup_size(std::uint32_t lanes, std::uint32_t n_eq)
    {
        bs = lanes;
        n_iter = (nc + bs - 1u) / bs;
        sv_rounds = (n_eq + bs - 1u) / bs;
    }
};

// ---- Which members come from the tape and which are recomputed from LDS-resident jets of the inputs (input_jets()). ----
struct block_input_jets {
    std::vector<char> recomp;            // per stored member: recomputed, not on the tape
    std::vector<char> ext_used;          // per external input: its jet is kept in LDS
    std::vector<std::uint32_t> ej_slots; // distinct slab slots of the external inputs with LDS jets
    std::vector<std::uint32_t> ej_index; // [x * nc + c] -> index into ej_slots
    std::uint32_t n_ej = 0;
    std::vector<std::uint32_t> tape_row; // per stored member: its row block on the tape
    std::uint32_t n_tape = 0;
};

// ---- The __device__ tables of the module, in the order they are emitted. ----
struct block_tables {
    std::ostringstream tbl;
    std::vector<std::pair<std::string, std::size_t>> utbl_list; // (name, entries) of the index tables
    std::string ut;                                             // their element type
    void emit_utbl(const std::string &name, const std::vector<std::uint32_t> &v);
    void emit_dtbl(const std::string &name, const std::vector<double> &v);
};

// ---- The pair phase: parameters (pair_parameters()), descriptor layout (pair_descriptors()), merged glue, declarations. ----
struct pair_phase {
    bool on = false; // the body of the kernel is the pair phase
    std::uint32_t R = 0; // rounds per lane (n_iter)
    std::uint32_t T = 0; // index pairs (slots) of the highest order
    std::uint32_t P = 0; // the order
    std::uint32_t M = 0, hand = 1, G = 0, D = 1;
    bool two_waves = false, lean = false, recip = false, reg_high = false, reg_high_br = false, il_tape = false,
         packed_idx = false, fuse_last = false, dbuf = false, xpf = false, hoist = false, keepdz = false, nopp = false;
    int exp_mode = 0;
    // Tape rows of the two members (r2 and its power), bytes per tape row; bytes per row of the input jets and its row of
    // order 0; the exponent of the power and exponent + 1.
    std::uint64_t arow0 = 0, brow0 = 0, rowb = 0, ejrow = 0, ej0b = 0;
    double ex = 0, e1 = 0;
    int io_of[3] = {-1, -1, -1}; // output index of the three products
    // Descriptor layout (pair_descriptors()): word / shift / constant of the byte offset of every external input, constants
    // of the output slots; compact: 2 words per cluster.
    std::vector<std::uint32_t> ex_word, ex_shift, ex_delta;
    std::uint32_t out_delta[3] = {0u, 0u, 0u};
    bool compact = false;
    std::uint32_t n_dq = 0, n_dw = 0; // words holding input offsets, words per cluster
    // Merged sum levels (pair_merged_glue()).
    struct merged_sums {
        std::vector<std::size_t> groups;
        std::vector<std::uint32_t> nodes;
        std::uint32_t nargs = 0;
    };
    std::map<std::uint32_t, merged_sums> merged;
    std::vector<char> group_merged;
    std::set<std::uint32_t> packed_levels;
    std::set<std::size_t> q_groups;
    std::ostringstream decl; // kernel-lifetime declarations of the pair phase
};

inline std::string U(std::uint64_t x)
{
    return std::to_string(x) + "u";
}
inline std::string S(std::uint32_t x)
{
    return std::to_string(x);
}
inline std::string nm2(const char *b, std::uint32_t i, std::uint32_t r)
{
    return std::string(b) + "_" + std::to_string(i) + "_" + std::to_string(r);
}

struct block_gen : block_geometry, block_input_jets, block_tables, pair_phase {
    const taylor_program &p;
    const emit_options &opts;
    emit_refusal &why_not;
    const block_switches sw;
    const std::uint32_t n_eq, order;
    ssa_emitter e;
    std::ostringstream &os; // the step body, through the SSA emitter
    std::ostringstream src; // the module
    std::string body;
    std::uint64_t per_block = 0; // doubles of scratch per workgroup
    std::uint32_t wpb = 0;       // wavefronts per workgroup

    block_gen(const taylor_program &p, const emit_options &opts, emit_refusal &why_not);

    // Stages, in the order emit_block() calls them; a stage which refuses returns false (plan(), input_jets(): with why_not
    // set; pair_phase_applicable(), pair_parameters(): the generic cluster phase takes over).
    bool plan(), input_jets();
    void base_tables();
    bool pair_phase_applicable();
    void begin_body(), generic_body();
    bool pair_parameters();
    void pair_descriptors(), pair_merged_glue(), pair_fused_last_level(), pair_lds_mirrors(), pair_order0(),
        pair_glue_levels(std::uint32_t k), pair_recursion(bool dyn), pair_order_loop();
    void module_text();
    emitted_module result();

    // Parts of the stages.
    void pad_output_blocks(), permute_clusters();
    void emit_cluster(std::uint32_t k), emit_glue_group(std::size_t g, std::uint32_t k);
    std::vector<std::uint32_t> bank_aware_lane_order(const std::vector<std::uint32_t> &nodes, std::uint32_t nargs) const;
    void pair_glue_level_staged(std::uint32_t lev, std::uint32_t k);
    void pair_resolve_pipeline(std::uint32_t hand_dflt);
    void lds_step(std::uint32_t i, std::uint32_t r, std::uint32_t set), tape_loads(std::uint32_t i, std::uint32_t r0, std::uint32_t r1),
        pair_group(std::uint32_t r0, std::uint32_t r1, std::uint32_t gi), pair_group_finish(std::uint32_t r0, std::uint32_t r1),
        pair_group_prefetch(std::uint32_t r1);

    // Emission helpers.
    void sync() { os << "__syncthreads();\n"; }
    std::string take_os() // (what has been written to the step body since the last call)
    {
        auto t = os.str();
        os.str("");
        os.clear();
        return t;
    }
    std::uint32_t oslot_of(std::uint32_t c, int x) const
    {
        return static_cast<std::uint32_t>(pl.slot_of[pl.clusters[c][pl.out_pos[static_cast<std::uint32_t>(x)]]]);
    }
    // Names of the pair phase: pipeline registers of slot i (set i % (D + 1)) and round r; cross-group prefetch registers;
    // the raw LDS values of a step (q: 0 = row i, 1 = row p).
    std::string gname(const char *b, std::uint32_t i, std::uint32_t r) const { return std::string(b) + S(i % (D + 1u)) + "_" + S(r); }
    static std::string xname(const char *b, std::uint32_t i, std::uint32_t q) { return std::string(b) + S(i) + "_" + S(q); }
    static std::string raw(std::uint32_t set, std::uint32_t q, std::uint32_t c, std::uint32_t side)
    {
        return "w" + S(set) + "_" + S(q) + S(c) + S(side);
    }
    // The byte offset of input x / the slab slot of output q / the cluster index of the lane's cluster in round r, as
    // expressions; the statements which load the descriptors of round r and unpack them.
    std::string ex_expr(std::uint32_t x, std::uint32_t r) const, out_expr(std::uint32_t q, std::uint32_t r) const, cl_expr(std::uint32_t r) const;
    void desc_loads(std::uint32_t r), unpack_ex(std::uint32_t r), unpack_out(std::uint32_t r);
    void diff(const std::string &name, std::uint32_t c, const std::string &row);
    void store_out(const std::string v[3]);
};

} // namespace heyoka_amd::block_detail
