// Internal launch interface between the kernel translation units (*.hip) and the C-ABI layer (boojum_hip.cpp).
// Not part of the public boundary (that is include/boojum_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include "callee_words.h"
#include "opening_args.h"
#include "term_io.h"
#include <stddef.h>
#include <stdint.h>
#include <string>

namespace bj {
typedef uint64_t u64;

// The environment switches of DESIGN.md §3 (A/B plans and test hooks; none changes a result), read ONCE — by the first
// bj_ctx_create of the process, under std::call_once — and never again on a proof path: no getenv races with a host thread's
// setenv, no per-proof lookups, and every context of a process (one per GPU, each on its own host thread) sees the same plan.
// bj_env_reload() re-reads them for tests that exercise both sides of a switch in one process (not thread-safe by contract).
struct EnvConfig {
    bool ntt_two_pass = true;           // BJ_NTT_TWO_PASS=0: 2^22-point transforms as 4 + 8 + 10 rounds instead of 10 + 12
    bool mono_tiled = true;             // BJ_MONO_TILED=0: bj_prove keeps 2^22-row monomials in natural order (inverse transforms end in a bit-reversal pass)
    bool gate_no_aot = false, gate_no_fuse = false, gate_no_jit = false;
    bool gates_windowed = true;         // BJ_GATES_WINDOWED=0: per-gate kernel for the hand-written kinds
    bool prove_no_absorb = false;
    bool setup_lean = false;            // BJ_SETUP_LEAN: a single-device setup created while it is set drops its LDE once the tree stands; sampled per setup
    bool proof_lean = false;            // BJ_PROOF_LEAN: a single-device proof keeps no LDE of its witness and stage-2 oracles: monomials, trees and one coset buffer each; sampled when a proof starts
    bool copy_perm_wide_k = false;      // BJ_COPY_PERM_WIDE_K: quotient_copy_perm with 64-bit non-residue products even when they fit 32 bits (A/B, tests)
    bool prove_uniform_groups = false;   // BJ_PROVE_UNIFORM_GROUPS: equal groups of G columns, one multi-block absorption run per group (round 4's GROUPING only: its launches absorbed eight columns each)
    bool async_stagger = true;           // BJ_ASYNC_STAGGER=0: bj_prove_async lanes start whenever they are given work (A/B)
    int async_mode = -1;                 // BJ_ASYNC_MODE: what a bj_prove_async lane does while its sibling proves: -1 by witness size (default), 0 bj_prove as is (+ stagger), 1 whole witness first, 2 groups + one hash
    bool async_debug = false;            // BJ_ASYNC_DEBUG: a bj_prove_async lane reports each proof it ran on stderr, and each submission the rung it was admitted on
    size_t hbm_budget_bytes = 0;         // BJ_HBM_BUDGET_BYTES (decimal; 0 or unset: no cap): the most a context and its bj_prove_async lanes may hold in arenas, staging, scratch and tables when a submission is admitted (async_admission.h)
    bool peer_debug = false;             // BJ_PEER_DEBUG: the peer transport traces its bulk exchanges on stderr
    int peer_test_fail_rank = -1;        // BJ_PEER_TEST_FAIL_RANK: test hook, this rank of the peer transport pretends it could not export its mailbox
    unsigned prove_h2d_group = 8;
    unsigned verify_threads = 8;         // BJ_VERIFY_THREADS (1..16): host threads of bj_verify_batch; never sized by the machine's core count
    size_t nodes_lanepar_max = 16384;
    std::string jit_cache_dir, rccl_lib;
};
const EnvConfig &env();
void env_reload();


// ntt.hip
void launch_twiddles(u64 *d_out, unsigned log_n, bool inverse, hipStream_t s);
void launch_round_scales(u64 *d_out, const u64 *h_shifts, unsigned n_cosets, unsigned log_n, hipStream_t s);
// What every NTT pass launcher is given: the columns it reads and writes, the twiddle table and the shape of the batch.
struct NttIo {
    const u64 *in;
    u64 *out;
    const u64 *tw;            // bit-reversed twiddle table
    const u64 *round_scale;   // [n_cosets][32] per-round twiddle scale, or nullptr (plain subgroup transform)
    unsigned log_n, n_cols, n_cosets;
    size_t in_col_stride;     // elements between input columns
    size_t in_coset_stride;   // 0 when every coset reads the same input column (the first pass), n when in place
    size_t out_col_stride;    // elements between output columns (each column holds n_cosets * n outputs)
    bool inverse;             // tw is the inverse root's table: the register steps run the inverse 16th roots of unity
};
// Runs the plan of ntt_plan.h for 1..64 cosets.  d_front_table: BJ_FRONT_TABLE_WORDS words of device scratch for the twiddle table
// of the two-pass plan; tiled_in: the caller's columns are in the tiled layout (two-pass plan only); skip_last: stop in front of
// the plan's last pass (the caller runs its own in its place); inverse: d_tw is the table of the inverse root (launch_twiddles)
constexpr size_t BJ_FRONT_TABLE_WORDS = 64 * 1024;
void launch_ntt_passes(const u64 *d_in, u64 *d_out, const u64 *d_tw, const u64 *d_round_scale, unsigned log_n,
                       unsigned n_cols, unsigned n_cosets, size_t in_col_stride, size_t out_col_stride, hipStream_t s,
                       u64 *d_front_table, bool tiled_in = false, bool skip_last = false, bool inverse = false);
// true when launch_ntt_passes would take the two-pass plan for these arguments (the only plan that reads the tiled layout)
bool ntt_two_pass_applies(const u64 *d_in, const u64 *d_out, unsigned log_n, size_t in_col_stride, size_t out_col_stride);
void launch_bitrev_scale(const u64 *d_in, u64 *d_out, unsigned log_n, unsigned n_cols, size_t in_col_stride,
                         size_t out_col_stride, u64 scale, u64 step, hipStream_t s);
void launch_canonicalize(u64 *d, size_t n, hipStream_t s);
void launch_field_op(int op, const u64 *a, const u64 *b, u64 *out, size_t n, hipStream_t s);

// ntt_r16.hip (register-radix-16 passes)
void launch_ntt_local12(const NttIo &io, unsigned rounds /* 12, or 10 / 9 behind launch_ntt_first4 / first5 */, hipStream_t s);
void launch_ntt_strided(const NttIo &io, unsigned r0, unsigned rounds /* 8 or 4 */, hipStream_t s);
void launch_ntt_first4(const NttIo &io, hipStream_t s);   // 16-byte accesses: ntt_aligned16 columns only
void launch_ntt_first5(const NttIo &io, hipStream_t s);
// first ten rounds of all cosets (log_n == 22, ntt_aligned16 columns); d_table: n_cosets * 1024 words of device scratch
void launch_ntt_front10(const NttIo &io, u64 *d_table, bool tiled_in, hipStream_t s);
// 2^22-word columns in the tiled layout (tiled_layout.h: tiled_index): last pass of an inverse transform storing it, re-layout kernel
void launch_ntt_local12_pair_tiled(const u64 *in, u64 *out, const u64 *tw, const u64 *tw_scaled /* tw[j] * scale, j < 2^21 */, u64 scale,
                                   unsigned n_cols, size_t in_col_stride, size_t out_col_stride, hipStream_t s);
void launch_scale_table(const u64 *in, u64 *out, size_t count, u64 scale, hipStream_t s);
void launch_tiled_permute(const u64 *in, u64 *out, unsigned n_cols, size_t in_col_stride, size_t out_col_stride, bool to_tiled, hipStream_t s);

// tree_hash.hip: the Merkle-tree entry points, dispatched on hasher = BJ_HASHER_* (what each hasher contributes: tree_plan.h)
void launch_tree_leaves(int hasher, const u64 *d_base, size_t col_stride, const u64 *const *d_col_ptrs, unsigned n_cols,
                        size_t num_leaves, u64 *d_digests, hipStream_t s);
void launch_tree_leaves_chunked(int hasher, const u64 *d_src0, const u64 *d_src1, unsigned n_srcs, unsigned log_e,
                                size_t num_leaves, u64 *d_digests, hipStream_t s);
void launch_tree_node_layers(int hasher, u64 *d_tree, size_t num_leaves, size_t cap_size, hipStream_t s);
// group-wise absorption for the algebraic hashers, BJ_HASHER_POSEIDON2 / BJ_HASHER_POSEIDON: one absorption run of a group of
// columns per leaf; d_capacity [4][num_leaves] carries the sponge between the groups
void launch_tree_leaves_absorb(int hasher, const u64 *d_base, size_t col_stride, unsigned n_cols, size_t num_leaves,
                               u64 *d_capacity, u64 *d_digests, bool first, bool last, hipStream_t s);
// poseidon2.hip, poseidon1.hip: the bare permutation on n_states 12-word states
void launch_poseidon2_permute_states(u64 *d_states, size_t n_states, hipStream_t s);
void launch_poseidon1_permute_states(u64 *d_states, size_t n_states, hipStream_t s);
// tree_hash.hip: proof of work of runner BJ_POW_* over nonces [base, base + count): atomicMin of the valid ones into *d_result
// (pre-set to ~0)
void launch_pow(int pow_runner, const u64 *seed5, unsigned pow_bits, u64 base, u64 count, u64 *d_result, hipStream_t s);

// fri.hip
// fold by 2^k (k = 1..3) in one launch; j0: the global output index of local output 0 (a shard's part of an oracle)
void launch_fri_fold_step(const u64 *d_c0, const u64 *d_c1, size_t len, unsigned k, u64 *d_o0, u64 *d_o1,
                          const u64 *d_roots, u64 coset_inv, u64 ch0, u64 ch1, hipStream_t s, size_t j0 = 0);
// stage2.hip and quotient.hip: the term kernels of rounds 2 and 3, given launch descriptors (term_io.h).
// d_tmp: copy_perm_stage2_scratch_words(ceil(V / chunk), n) words; d_z [2][n], d_partials [(n_chunks - 1)][2][n]
void launch_copy_perm_stage2(const CopyPermArg &cp, u64 *d_tmp, u64 *d_z, u64 *d_partials, hipStream_t s);
void launch_lookup_polys(const LookupArg &l, unsigned log_n, u64 *d_A, u64 *d_B, hipStream_t s);
// the hand-written kinds of a gate list (gate_list.h) in one launch, OVERWRITING out; the other kinds only keep their alpha powers
struct GateShape;
void launch_quotient_gates(const GateCols &cols, const GateShape *gates, unsigned n_gates, const TermSink &out, hipStream_t s);
// out += the lookup terms; d_A [2 * reps] and d_B [2] columns at s2_stride
void launch_quotient_lookup(const LookupArg &l, const u64 *d_A, const u64 *d_B, size_t s2_stride, const TermSink &out, hipStream_t s);
// out = (out + alpha_L1 * (z - 1) * L1~ + copy-permutation chain) / (x^n - 1) on points [I0, I0 + out.points) of the LDE of 2^log_L
// cosets; stage2: z and the partial products; out.d_alphas: the chunk powers (the power behind h_alpha_l1's);
// d_inv_xm1: 1 / (x - 1) per local point, or null (computed in the kernel)
void launch_quotient_copy_perm(const CopyPermArg &cp, Cols stage2, unsigned log_L, const u64 *h_alpha_l1, const TermSink &out, size_t I0,
                               const u64 *d_inv_xm1, hipStream_t s);
void launch_inv_x_minus_one(const u64 *d_tw_fwd, size_t Q, size_t I0, u64 *d_out, hipStream_t s);
bool launch_combine_residues(const u64 *d_residues, unsigned W, size_t E, unsigned n_cols, const u64 *h_a, u64 *d_out, hipStream_t s);
void launch_gather_rows(const u64 *d_base, size_t col_stride, unsigned n_cols, const u64 *d_idx, unsigned n_idx,
                        u64 *d_out, hipStream_t s);
void launch_merkle_paths(const u64 *d_tree, size_t num_leaves, unsigned depth, const u64 *d_idx, unsigned n_idx,
                         u64 *d_out, hipStream_t s);
void launch_gather_fri_leaves(const u64 *d_c0, const u64 *d_c1, unsigned log_e, const u64 *d_leaf_idx, unsigned n_idx,
                              u64 *d_out, hipStream_t s);
// gate_poseidon.hip: out += the gate's terms; G.kind: BJ_GATE_POSEIDON2_FLATTENED or BJ_GATE_POSEIDON_FLATTENED.  Quotient mode only:
// out.d_alphas must not be null (the kernels have no stand-alone term mode)
void launch_quotient_poseidon_gate(const GateShape &G, const GateCols &cols, const TermSink &out, hipStream_t s);
// openings.hip
void launch_barycentric_weights(u64 *d_w0, u64 *d_w1, const u64 *d_tw_fwd, unsigned log_n, u64 coset, const u64 *at,
                                hipStream_t s);
void launch_barycentric_eval(const u64 *const *d_col_ptrs, unsigned n_cols, size_t n, const u64 *d_w0, const u64 *d_w1,
                             u64 *d_partials, u64 *d_out, hipStream_t s);
void launch_linear_combination(const u64 *const *d_col_ptrs, const u64 *d_coefs, unsigned n_cols, size_t n, u64 *d_out0,
                               u64 *d_out1, hipStream_t s);
// d_out[j][c] = sum_i mono_c[i] * x_j^i for every column c (n_cols of 2^log_n coefficients at col_stride; tiled: in the tiled
// layout, 2^22 only) and every j < n_idx, x_j the LDE point of leaf I0 + d_idx[j] (the DEEP kernels' x_I): what gather_rows would
// read at d_idx[j] from the columns' LDE, canonical, same order.  One launch for all queries
void launch_eval_monomials_at(const u64 *d_mono, size_t col_stride, unsigned n_cols, unsigned log_n, bool tiled, const u64 *d_tw_fwd, size_t I0,
                              const u64 *d_idx, unsigned n_idx, u64 *d_out, hipStream_t s);
// the opening sets of a column list (opening_args.h; at most DEEP_MAX_SETS) in one launch; d_ptrs / d_coefs: the list's two parts
// on the device
void launch_deep_accumulate_multi(const ColumnSet *sets, unsigned n_sets, const u64 *const *d_ptrs, const u64 *d_coefs, size_t N,
                                  size_t I0, const u64 *d_tw_fwd, u64 *d_dst0, u64 *d_dst1, int accumulate, hipStream_t s);
// copy_check.hip: sigma words -> cell numbers with the decoding table of that file (d_table); the one-pass check of a setup's
// sigma columns against the variables (both [num_vars][n] at stride n) and its second pass for a sigma that is no permutation
void launch_sigma_cells(const u64 *d_sigmas, size_t sig_stride, unsigned num_vars, unsigned log_n, const u64 *d_table, uint32_t *d_cells,
                        size_t cell_stride, u64 *d_ctr, hipStream_t s);
void launch_copy_check(const u64 *d_sigmas, const u64 *d_vars, unsigned num_vars, unsigned log_n, const u64 *d_table, uint32_t *d_seen,
                       uint32_t *d_multi, u64 *d_ctr, hipStream_t s);
void launch_copy_shared_target(const u64 *d_sigmas, unsigned num_vars, unsigned log_n, const u64 *d_table, const uint32_t *d_multi, u64 *d_ctr,
                               hipStream_t s);
// witness_values.hip: witness_gather_kernel, d_cells[i] = d_values[d_placement[i]] for i < count (0 for PLACEMENT_NONE; 0 and *d_bad
// raised for an index at or beyond n_values); the grid is sized to the CU count and strides, one sweep of it covers
// witness_gather_sweep_cells().  launch_widen_counters: d_column[i] = d_counters[i] for i < n_counters, 0 up to n.
void launch_witness_gather(const uint32_t *d_placement, const u64 *d_values, size_t n_values, u64 *d_cells, size_t count, unsigned *d_bad,
                           hipStream_t s);
size_t witness_gather_sweep_cells();
void launch_widen_counters(const uint32_t *d_counters, size_t n_counters, u64 *d_column, size_t n, hipStream_t s);
}  // namespace bj
