// Rewrites of the INTERNAL program (program_rewrite.cpp). The planner of the wave-cluster and block kernels accepts a narrow
// set of shapes; these passes bring a decomposition into one of them. The decomposition the user sees is never touched:
// emit_hip_module() (hip_emit_select.cpp) generates the code from the rewritten copy and exposes its text as
// emitted_module::internal_program. Every pass returns false - and leaves `out` unspecified - when it does not apply.
#pragma once

#include <cstdint>

#include "decompose.hpp"

namespace heyoka_amd
{

// State variables as history operands. The planner groups a nonlinear node with the u variables whose whole history it
// needs; a *state variable* in that position (model::np1body: |r_i|^2 = sum_sq(x_i, y_i, z_i), x_i * |r_i|^-3) cannot be
// a member of a cluster. This transformation
//   - gives every state variable s read by a cluster member a glue copy g_s = sum(s),
//   - gives every state variable in history position an alias a_s = g_s - z_s (z_s: a constant-zero node of its own),
//     an ordinary cluster member with the shape of the coordinate differences of a pair cluster, and
//   - rewires the members to g_s / a_s,
// so that heliocentric and pair clusters are isomorphic and sit at the same dependency level (both read level-1 glue).
// The values are unchanged (s + nothing, s - 0). Returns false if the program needs no alias.
bool add_state_aliases(const taylor_program &p, taylor_program &out);

// Clusters which differ by an *elided unit factor*. model::nbody() scales r^-3 by G m_j before the three products of a
// pair; when that factor is exactly 1 (unit masses in G = 1 units) the scaling node is not there and the products read the
// pow directly, while the pairs of the same system with another factor (-G m_i = -1 towards a test particle, other
// masses) keep it: the pair clusters are then neither isomorphic nor sub-shapes of each other. This pass restores the
// missing member in the INTERNAL program (the user-visible decomposition is untouched): every pow node which is read by
// products with a variable factor but by no scaling product `c * pow`, in a program where other pow nodes are read
// through such a scaling, gets `s = 1.0 * pow` right behind it, and its product readers read s (x * 1.0 is exact: no
// value changes). Returns false if there is nothing of that kind.
bool insert_unit_scalings(const taylor_program &p, taylor_program &out);

// Accelerations as flat sums of scaled pair products. model::nbody() writes the acceleration of a body as whatever its
// masses let the expression system fold: with distinct numerical masses a plain sum over the partners, each term a product
// d * (G m r^-3) or its "reaction" c * (d * (G m r^-3)) - the shape the one-lane-per-pair kernel is built for -, but with
// EQUAL masses the reactions become negations and the sums of a body turn into sum / sub / -1 * sum trees whose kind differs
// from body to body (default masses: src/model/nbody.cpp:95-130, the grouped branch), and with REPEATED masses the reactions
// are glue nodes of their own in front of the sums: two glue levels. The lanes of a glue round execute one instruction
// stream, so those systems fell to the lane-pair / first-generation kernels (1.5e8 ... 5.5e8 system-steps/s against 7.9e8).
// This pass rewrites the INTERNAL program (the user-visible decomposition is untouched): the definition of every state
// variable which is a linear tree - sum, sub, prod(number, .) - over products of two variables is flattened into
// sum_j c_j p_j; every product keeps the appearance with coefficient +1 as the direct one, the other one becomes a node
// prod(c, p) right behind it (the reaction), and the acceleration becomes ONE sum node over its terms in the order of the
// flattened tree. The result has the shape of the distinct-mass decomposition. NOTE: the additions of an acceleration are
// re-associated (one pairwise sum over all the terms instead of the tree of the expression) and nested constant factors are
// multiplied on the host: the jets of the rewritten program agree with the decomposition to rounding, not bit for bit -
// the one rewrite of this family with that property (tests: 1e3 eps on the jets of the internal program).
// Returns false if the program does not have that form or nothing would change.
bool linearise_accelerations(const taylor_program &p, taylor_program &out);

// Distinct masses in a pair-interaction system: model::nbody() scales the power of the distance ONCE per pair
// (s = c * r^-3), multiplies the coordinate differences by it and derives the reactions from those products - scaling,
// scaled products and reactions are members of the pair's cluster. The v2 cluster phase of block mode (rolled order loop,
// rows in registers, index-pair convolutions: the kernel of model::nbody(64) with its equal masses) wants the clusters of the
// EQUAL-mass system: differences, sum of squares, power, three unit products. This pass rewrites the INTERNAL program (the
// user-visible decomposition is untouched): every product d * s reads r^-3 directly, a node c * (d * r^-3) placed right
// behind it takes its place for the sums which read it, a reaction c' * (d * s) becomes (c' c) * (d * r^-3), the scaling node
// goes. Equal to the decomposition to rounding (c (d r^-3) against d (c r^-3); the product of the two constants is formed in
// double precision). Returns false if nothing has that shape.
bool externalise_scalings(const taylor_program &p, taylor_program &out);

// Clusters which SHARE cheap linear members. The sum of squares at the head of a distance cluster reads coordinate
// differences `c - x` / `x - c` of ONE variable and a number; when several clusters have the same difference (fixed
// centres / mascons with a repeated coordinate) common-subexpression elimination gives them ONE node, and a coordinate
// which is zero turns `0 - x` into `-1 * x` (model::fixed_centres with a centre at the origin, a mascon on an axis): the
// clusters then overlap or differ in the kind of a member, and the cluster planner gives up ("clusters are not
// isomorphic": table stepper, 100x slower). This pass rewrites the INTERNAL program (the user-visible decomposition is
// untouched): every sum of squares all of whose arguments are such differences gets PRIVATE copies of them, placed right
// in front of it in argument order, negations written as `-0.0 - x` (bit for bit the same value as `-1 * x`, signed
// zeros and NaNs included: -0 - (+0) = -0, -0 - (-0) = +0); the products of the cluster (difference times the -
// possibly scaled - power of the sum of squares) read the copies; originals which nobody reads any more are dropped.
// A few redundant subtractions per step buy the cluster kernels. Returns false if nothing of that kind is found.
bool privatise_cluster_inputs(const taylor_program &p, taylor_program &out);

// Clusters of different shapes. When every cluster is a *sub-shape* of the largest one (model::nbody with massless
// bodies: the pairs with a test particle lack the three reaction products of the massive-massive pairs), the smaller
// clusters are padded in the INTERNAL program (the user-visible decomposition is untouched, like add_state_aliases())
// with the members they lack - same kinds and operands as in the template, results nobody reads - so that all the
// clusters are isomorphic and the wave-cluster steppers apply instead of the table-driven one. The embedding of a
// cluster into the template is found by backtracking over the (small) member lists: kinds, argument structure
// (member -> member edges, consistent external inputs, structural numbers) and hidden dependencies must match.
// Returns false if the program is not of that kind.
bool pad_clusters(const taylor_program &p, std::uint32_t order, taylor_program &out);

} // namespace heyoka_amd
