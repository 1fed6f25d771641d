// Blake2s-256 Merkle hashing for gfx950 — the tree hasher of the reference's non-recursive configuration
// (`impl TreeHasher<F> for blake2::Blake2s256`, src/cs/oracle/mod.rs:179-245; bench `run_sha256_prover_non_recursive`,
// gadgets/sha256/mod.rs:265-270).  The hash itself is RFC 7693 (crate blake2 0.10, unkeyed, 32-byte digest):
//   leaf  = Blake2s( le64(canonical(e_0)) || le64(canonical(e_1)) || ... )        one update per element
//   node  = Blake2s( left[32] || right[32] )
// lane = leaf / node, the 8-word chaining value and the 16-word message block live in VGPRs; a block is 8 field
// elements, i.e. 8 coalesced column loads.  Pure 32-bit add/xor/rotate (v_alignbit) work: ~1.3 k VALU instructions per
// 64-byte block against ~14 k for one Poseidon2 permutation over the same 8 elements.
// Digests are stored as four little-endian u64 words = the 32 digest bytes in memory order (never canonicalised).
// The per-lane kernel bodies (tree leaves through their three doors, node layers, proof of work) are the plan of byte_tree.h,
// shared with keccak.hip; the fetches, the launch helpers and the entry this file contributes to the hasher dispatch of
// tree_hash.hip are in tree_plan.h.  Here: the compression, the policy with the ONE block loop (8 words + the byte counter t),
// the entry points.
#include "gl.h"
#include "kernels.h"
#include "byte_tree.h"
#include "verify_open.h"

using gl::u64;
using gl::u32;

namespace bj {
namespace {

__device__ __constant__ const u32 B2S_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                                               0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
__device__ __constant__ const unsigned char B2S_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

__device__ __forceinline__ u32 rotr(u32 x, unsigned n) { return __builtin_amdgcn_alignbit(x, x, n); }

struct B2s {
    u32 h[8];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = B2S_IV[i];
        h[0] ^= 0x01010020u;   // digest length 32, no key, fanout 1, depth 1
    }
    // one compression (RFC 7693 §3.2); t = bytes hashed so far including this block
    __device__ __forceinline__ void compress(const u32 (&m)[16], u64 t, bool last) {
        u32 v[16];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            v[i] = h[i];
            v[8 + i] = B2S_IV[i];
        }
        v[12] ^= (u32)t;
        v[13] ^= (u32)(t >> 32);
        if (last) v[14] = ~v[14];
#define B2S_G(a, b, c, d, x, y)                 \
    v[a] = v[a] + v[b] + (x);                   \
    v[d] = rotr(v[d] ^ v[a], 16);               \
    v[c] = v[c] + v[d];                         \
    v[b] = rotr(v[b] ^ v[c], 12);               \
    v[a] = v[a] + v[b] + (y);                   \
    v[d] = rotr(v[d] ^ v[a], 8);                \
    v[c] = v[c] + v[d];                         \
    v[b] = rotr(v[b] ^ v[c], 7);
#pragma unroll
        for (int r = 0; r < 10; r++) {
            const unsigned char *s = B2S_SIGMA[r];
            B2S_G(0, 4, 8, 12, m[s[0]], m[s[1]])
            B2S_G(1, 5, 9, 13, m[s[2]], m[s[3]])
            B2S_G(2, 6, 10, 14, m[s[4]], m[s[5]])
            B2S_G(3, 7, 11, 15, m[s[6]], m[s[7]])
            B2S_G(0, 5, 10, 15, m[s[8]], m[s[9]])
            B2S_G(1, 6, 11, 12, m[s[10]], m[s[11]])
            B2S_G(2, 7, 8, 13, m[s[12]], m[s[13]])
            B2S_G(3, 4, 9, 14, m[s[14]], m[s[15]])
        }
#undef B2S_G
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
    }
    __device__ __forceinline__ void digest(u64 (&d)[4]) const {
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = gl::pack(h[2 * k], h[2 * k + 1]);
    }
};

// the hash policy of byte_tree.h / verify_open.h
struct Blake2sTree {
    // 8 canonical words per 64-byte block; an empty message is one (final) zero block
    template <typename W>
    static __device__ __forceinline__ void leaf(W word, unsigned n, u64 (&d)[4]) {
        B2s st;
        st.init();
        const unsigned n_blocks = n ? (n + 7) / 8 : 1;
        for (unsigned b = 0; b < n_blocks; b++) {
            u32 m[16];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const unsigned c = b * 8 + k;
                const u64 v = c < n ? gl::canon(word(c)) : 0;
                m[2 * k] = gl::lo32(v);
                m[2 * k + 1] = gl::hi32(v);
            }
            const bool last = b + 1 == n_blocks;
            st.compress(m, last ? (u64)n * 8 : (u64)(b + 1) * 64, last);
        }
        st.digest(d);
    }
    // exactly one 64-byte block
    static __device__ __forceinline__ void node(const u64 (&l)[4], const u64 (&r)[4], u64 (&d)[4]) {
        u32 m[16];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            m[2 * k] = gl::lo32(l[k]);
            m[2 * k + 1] = gl::hi32(l[k]);
            m[8 + 2 * k] = gl::lo32(r[k]);
            m[8 + 2 * k + 1] = gl::hi32(r[k]);
        }
        B2s st;
        st.init();
        st.compress(m, 64, true);
        st.digest(d);
    }
    // seed = 5 field elements = 40 bytes, so seed || nonce is one 48-byte block
    static __device__ __forceinline__ u64 pow_word(const u64 (&seed)[5], u64 nonce) {
        u32 m[16];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            m[2 * k] = gl::lo32(seed[k]);
            m[2 * k + 1] = gl::hi32(seed[k]);
        }
        m[10] = gl::lo32(nonce);
        m[11] = gl::hi32(nonce);
        m[12] = m[13] = m[14] = m[15] = 0;
        B2s st;
        st.init();
        st.compress(m, 48, true);
        return gl::pack(st.h[0], st.h[1]);
    }
};

// the plan of byte_tree.h around this hash
__global__ void __launch_bounds__(256)
blake2s_leaves_kernel(const u64 *base, size_t col_stride, const u64 *const *col_ptrs, unsigned n_cols, size_t num_leaves,
                      u64 *digests) {
    byte_leaves<Blake2sTree>(base, col_stride, col_ptrs, n_cols, num_leaves, digests);
}
__global__ void __launch_bounds__(256)
blake2s_leaves_chunked_kernel(const u64 *src0, const u64 *src1, unsigned n_srcs, unsigned log_e, size_t num_leaves,
                              u64 *digests) {
    byte_leaves_chunked<Blake2sTree>(src0, src1, n_srcs, log_e, num_leaves, digests);
}
__global__ void __launch_bounds__(256) blake2s_nodes_kernel(const u64 *children, u64 *parents, size_t num_parents) {
    byte_nodes<Blake2sTree>(children, parents, num_parents);
}
__global__ void __launch_bounds__(256) blake2s_pow_kernel(PowSeed seed, unsigned pow_bits, u64 base, u64 count, unsigned long long *result) {
    byte_pow<Blake2sTree>(seed, pow_bits, base, count, result);
}

}  // namespace

// bj_verify / bj_verify_batch: one (query, oracle) Merkle chain per lane over every proof of the launch, chain -> (proof, query)
// through the record table (verify_open.h)
__global__ void __launch_bounds__(VERIFY_OPEN_BLOCK) blake2s_verify_openings_kernel(VerifyOpenArgs A) { verify_open<verify_chain_bytes<Blake2sTree>>(A); }

TreeHasher blake2s_tree_hasher() {
    return {tree_leaves<blake2s_leaves_kernel>, tree_leaves_chunked<blake2s_leaves_chunked_kernel>, tree_nodes<blake2s_nodes_kernel>, nullptr,
            tree_verify_openings<blake2s_verify_openings_kernel>, tree_pow<blake2s_pow_kernel>};
}

}  // namespace bj
