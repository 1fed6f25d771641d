// What the four Merkle-tree hashers (poseidon2.hip, poseidon1.hip, blake2s.hip, keccak.hip) share: where a lane finds the
// words of its leaf, how a per-lane kernel is launched, and the entry each hasher contributes to the dispatch of tree_hash.hip:
// a hasher file names each of its kernels once, as the argument of the launcher of the slot it fills.
// How the words are absorbed (rate, padding, length tag) is each hasher's own.
#pragma once
#include "gl.h"
#include "verify_open.h"

namespace bj {
typedef uint64_t u64;

// word of column c for leaf I; columns are base + c * col_stride or come through a device array of column pointers.
// c is wave-uniform, so a wavefront reads 64 consecutive words of one column (512 B, coalesced).
__device__ __forceinline__ u64 leaf_word(const u64 *base, size_t col_stride, const u64 *const *col_ptrs, unsigned c, size_t I) {
    const u64 *p = col_ptrs ? col_ptrs[c] : base + (size_t)c * col_stride;
    return p[I];
}
// word idx of leaf j = src0[jE..(j+1)E) || src1[jE..(j+1)E), E = 2^log_e   (FRI oracles, merkle_tree.rs:176-386)
__device__ __forceinline__ u64 chunk_word(const u64 *src0, const u64 *src1, unsigned log_e, unsigned E, size_t j, unsigned idx) {
    const u64 *p = (idx >> log_e) == 0 ? src0 : src1;
    return p[j * E + (idx & (E - 1))];
}

// one lane per item, 256-lane workgroups
template <typename... Params, typename... Args>
inline void launch_1d(void (*kernel)(Params...), size_t n, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, args...);
}

// proof-of-work seed (5 field elements, 40 bytes) as a kernel argument
struct PowSeed {
    u64 w[5];
};

// a hasher's launchers, one table entry of tree_hash.hip
struct TreeHasher {
    void (*leaves)(const u64 *d_base, size_t col_stride, const u64 *const *d_col_ptrs, unsigned n_cols, size_t num_leaves,
                   u64 *d_digests, hipStream_t s);
    void (*leaves_chunked)(const u64 *d_src0, const u64 *d_src1, unsigned n_srcs, unsigned log_e, size_t num_leaves, u64 *d_digests,
                           hipStream_t s);
    void (*nodes)(const u64 *d_children, u64 *d_parents, size_t num_parents, hipStream_t s);   // one layer
    // one absorption run of a group of columns per leaf, d_capacity [4][num_leaves] carries the sponge between the groups;
    // null for the byte hashers
    void (*leaves_absorb)(const u64 *d_base, size_t col_stride, unsigned n_cols, size_t num_leaves, u64 *d_capacity, u64 *d_digests,
                          bool first, bool last, hipStream_t s);
    // bj_verify / bj_verify_batch: the (query, oracle) Merkle chains of every proof of a batch in one launch (verify_open.h)
    void (*verify_openings)(const VerifyOpenArgs &args, hipStream_t s);
    // proof of work over the nonces [base, base + count) (byte_tree.h); null for the algebraic hashers
    void (*pow)(const PowSeed &seed, unsigned pow_bits, u64 base, u64 count, u64 *d_result, hipStream_t s);
};
TreeHasher poseidon2_tree_hasher(), blake2s_tree_hasher(), keccak_tree_hasher(), poseidon1_tree_hasher();

// the launcher of each slot around the kernel K that fills it
template <auto K>
void tree_leaves(const u64 *d_base, size_t col_stride, const u64 *const *d_col_ptrs, unsigned n_cols, size_t num_leaves, u64 *d_digests,
                 hipStream_t s) {
    launch_1d(K, num_leaves, s, d_base, col_stride, d_col_ptrs, n_cols, num_leaves, d_digests);
}
template <auto K>
void tree_leaves_chunked(const u64 *d_src0, const u64 *d_src1, unsigned n_srcs, unsigned log_e, size_t num_leaves, u64 *d_digests,
                         hipStream_t s) {
    launch_1d(K, num_leaves, s, d_src0, d_src1, n_srcs, log_e, num_leaves, d_digests);
}
template <auto K>
void tree_nodes(const u64 *d_children, u64 *d_parents, size_t num_parents, hipStream_t s) {
    launch_1d(K, num_parents, s, d_children, d_parents, num_parents);
}
template <auto K>
void tree_leaves_absorb(const u64 *d_base, size_t col_stride, unsigned n_cols, size_t num_leaves, u64 *d_capacity, u64 *d_digests,
                        bool first, bool last, hipStream_t s) {
    launch_1d(K, num_leaves, s, d_base, col_stride, n_cols, num_leaves, d_capacity, d_digests, first, last);
}
// grid.y = oracle, grid.x * VERIFY_OPEN_BLOCK + lane = chain of that oracle over the whole batch
template <auto K>
void tree_verify_openings(const VerifyOpenArgs &A, hipStream_t s) {
    hipLaunchKernelGGL(K, dim3((A.n_chains + VERIFY_OPEN_BLOCK - 1) / VERIFY_OPEN_BLOCK, A.n_oracles), dim3(VERIFY_OPEN_BLOCK), 0, s, A);
}
template <auto K>
void tree_pow(const PowSeed &seed, unsigned pow_bits, u64 base, u64 count, u64 *d_result, hipStream_t s) {
    launch_1d(K, count, s, seed, pow_bits, base, count, (unsigned long long *)d_result);
}

}  // namespace bj
