// The Merkle-tree plan of the byte hashers, once: the bodies of the per-lane kernels of a hash over byte strings with a 32-byte
// digest, as templates over a hash policy H.  blake2s.hip and keccak.hip contribute their compression / permutation and the
// policy, and wrap each body in a __global__ kernel of their own name (the counterpart of sponge_tree.h).
//
//   H::leaf(word, n, d)        the ONE block loop of the hash: d = hash( le64(canonical(word(0))) || ... || le64(canonical(word(n-1))) ),
//                              word(c) any callable that gives raw word c of the message; n = 0 is the hash of the empty string
//   H::node(l, r, d)           d = hash( l[32 bytes] || r[32 bytes] )
//   H::pow_word(seed, nonce)   the first 8 digest bytes of hash( seed[40 bytes] || le64(nonce) ) as a little-endian word
//
// A leaf has three doors and all of them are H::leaf: the columns of a trace (leaf_word), the chunks of a FRI oracle (chunk_word)
// and the opened words of a query (verify_chain_bytes, verify_open.h).  Digests are four raw little-endian words = the 32 digest
// bytes in memory order, never canonicalised.  Mapping: one lane = one leaf, one parent node or one nonce; the hash state lives
// in VGPRs, c is wave-uniform in every door, so a wavefront's loads of a column are coalesced.
#pragma once
#include "tree_plan.h"

namespace bj {

__device__ __forceinline__ void byte_store_digest(u64 *digests, size_t i, const u64 (&d)[4]) {
    ulonglong2 *p = reinterpret_cast<ulonglong2 *>(digests + 4 * i);
    p[0] = make_ulonglong2(d[0], d[1]);
    p[1] = make_ulonglong2(d[2], d[3]);
}

// leaf I = hash of the canonical little-endian bytes of cols[0][I], cols[1][I], ...          (merkle_tree.rs:78-174)
template <typename H>
__device__ __forceinline__ void byte_leaves(const u64 *base, size_t col_stride, const u64 *const *col_ptrs, unsigned n_cols,
                                            size_t num_leaves, u64 *digests) {
    const size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= num_leaves) return;
    u64 d[4];
    H::leaf([=](unsigned c) { return leaf_word(base, col_stride, col_ptrs, c, I); }, n_cols, d);
    byte_store_digest(digests, I, d);
}

// leaf j = hash( src0[jE..(j+1)E) || src1[jE..(j+1)E) )                            (FRI oracles, merkle_tree.rs:176-386)
template <typename H>
__device__ __forceinline__ void byte_leaves_chunked(const u64 *src0, const u64 *src1, unsigned n_srcs, unsigned log_e,
                                                    size_t num_leaves, u64 *digests) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    const unsigned E = 1u << log_e;
    u64 d[4];
    H::leaf([=](unsigned e) { return chunk_word(src0, src1, log_e, E, j, e); }, n_srcs * E, d);
    byte_store_digest(digests, j, d);
}

// node layer: parent i = hash( children[2i] || children[2i+1] )                              (oracle/mod.rs:179-312)
template <typename H>
__device__ __forceinline__ void byte_nodes(const u64 *children, u64 *parents, size_t num_parents) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_parents) return;
    const ulonglong2 *c = reinterpret_cast<const ulonglong2 *>(children + 8 * i);
    const ulonglong2 a = c[0], b = c[1], e = c[2], f = c[3];
    const u64 l[4] = {a.x, a.y, b.x, b.y}, r[4] = {e.x, e.y, f.x, f.y};
    u64 d[4];
    H::node(l, r, d);
    byte_store_digest(parents, i, d);
}

// Proof of work (impl PoWRunner for Blake2s256 / Keccak256, src/cs/implementations/pow.rs:50-230): the smallest nonce such that
// the first 8 digest bytes of hash(seed || le64(nonce)), read as a little-endian u64, have >= pow_bits trailing zeros.
// lane = nonce of [base, base + count); the minimum of the valid ones over the launch goes into *result (pre-set to ~0).
template <typename H>
__device__ __forceinline__ void byte_pow(const PowSeed &seed, unsigned pow_bits, u64 base, u64 count, unsigned long long *result) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64 nonce = base + i;
    const u64 first = H::pow_word(seed.w, nonce);
    const unsigned tz = first ? (unsigned)__builtin_ctzll(first) : 64u;
    if (tz >= pow_bits) atomicMin(result, (unsigned long long)nonce);
}

}  // namespace bj
