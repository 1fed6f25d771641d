// The Merkle-tree plan of the algebraic hashers, once: the bodies of the per-lane kernels of a sponge over Goldilocks with
// t = 12, rate 8 / capacity 4, as templates over the permutation (PERMUTE: state in any u64 words, state out weak words).
// poseidon2.hip and poseidon1.hip contribute their permutation and wrap each body in a __global__ kernel of their own name.
//
// Must equal the reference's CPU tree hasher bit for bit (as canonical residues):
//   sponge             src/algebraic_props/sponge.rs:224-346            overwrite absorption, zero-padded tail, no length tag
//   leaf / node hash   src/cs/oracle/mod.rs:114-176
//   tree               src/cs/oracle/merkle_tree.rs:78-174 (construct), 176-386 (chunked), 388-449 (node layers)
//
// Mapping: one lane = one leaf (or one parent node).  The 12-word sponge state lives in VGPRs for the whole leaf; round
// constants are wave-uniform and come through the scalar cache.
//
// Every leaf kernel has ONE call site of the permutation: with a second copy for the zero-padded tail block a Poseidon2 leaf
// kernel is 72 KB of code, more than the 64 KB instruction cache two CUs share; the tail's zeros are selected by wave-uniform
// conditions instead.  The same holds for the chunked leaves (FRI oracles, merkle_tree.rs:176-386), whose loop the two files
// write out around chunk_word (tree_plan.h) and sponge_store_digest.
#pragma once
#include "tree_plan.h"

namespace bj {

// digest = state[0..4] as canonical residues; 32 B per lane
__device__ __forceinline__ void sponge_store_digest(u64 *digests, size_t i, const u64 (&s)[12]) {
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(digests + 4 * i);
    d[0] = make_ulonglong2(gl::canon(s[0]), gl::canon(s[1]));
    d[1] = make_ulonglong2(gl::canon(s[2]), gl::canon(s[3]));
}

// leaf I = sponge(cols[0][I], cols[1][I], ...)                             (merkle_tree.rs:78-174)
template <void (*PERMUTE)(u64 (&)[12])>
__device__ __forceinline__ void sponge_leaves(const u64 *base, size_t col_stride, const u64 *const *col_ptrs, unsigned n_cols,
                                              size_t num_leaves, u64 *digests) {
    const size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= num_leaves) return;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = 0;
    for (unsigned c = 0; c < n_cols; c += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = c + k < n_cols ? leaf_word(base, col_stride, col_ptrs, c + k, I) : 0;
        PERMUTE(s);
    }
    sponge_store_digest(digests, I, s);
}

// A RUN of absorptions of the same sponge, for leaves whose columns arrive in groups (bj_prove: the witness comes over PCIe
// while the first groups are already being extended and hashed): state[8..12] <- what the previous group left in `capacity`
// ([4][num_leaves], zeros before the first group); then, eight columns at a time, state[0..8] <- the group's next elements
// (zero-padded in the last block of the last group), permute — every group but the last holds a multiple of eight columns;
// the last group writes the digest, the others their capacity words.  Group by group this is exactly sponge_leaves' loop.
template <void (*PERMUTE)(u64 (&)[12])>
__device__ __forceinline__ void sponge_leaves_absorb(const u64 *base, size_t col_stride, unsigned n_cols, size_t num_leaves,
                                                     u64 *capacity, u64 *digests, int first, int last) {
    const size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= num_leaves) return;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 4; k++) s[8 + k] = first ? 0 : capacity[(size_t)k * num_leaves + I];
    for (unsigned c = 0; c < n_cols; c += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = c + k < n_cols ? base[(size_t)(c + k) * col_stride + I] : 0;
        PERMUTE(s);
    }
    if (last) {
        sponge_store_digest(digests, I, s);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) capacity[(size_t)k * num_leaves + I] = s[8 + k];
    }
}

// node layer: parent i = perm(left || right || 0000)[0..4]                 (oracle/mod.rs:162-168)
template <void (*PERMUTE)(u64 (&)[12])>
__device__ __forceinline__ void sponge_nodes(const u64 *children, u64 *parents, size_t num_parents) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_parents) return;
    const ulonglong2 *c = reinterpret_cast<const ulonglong2 *>(children + 8 * i);
    const ulonglong2 a = c[0], b = c[1], e = c[2], f = c[3];
    u64 s[12] = {a.x, a.y, b.x, b.y, e.x, e.y, f.x, f.y, 0, 0, 0, 0};
    PERMUTE(s);
    sponge_store_digest(parents, i, s);
}

// the bare permutation on n_states 12-word states, canonical words out (transcript and test entry points of the C ABI)
template <void (*PERMUTE)(u64 (&)[12])>
__device__ __forceinline__ void sponge_permute_states(u64 *states, size_t n_states) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_states) return;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = states[12 * i + k];
    PERMUTE(s);
#pragma unroll
    for (int k = 0; k < 12; k++) states[12 * i + k] = gl::canon(s[k]);
}

}  // namespace bj
