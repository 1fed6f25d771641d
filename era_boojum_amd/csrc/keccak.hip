// Keccak-256 Merkle hashing for gfx950 — `impl TreeHasher<F> for sha3::Keccak256` (src/cs/oracle/mod.rs:247-312): the
// original Keccak padding (0x01 ... 0x80, NOT the 0x06 of FIPS-202 SHA3-256), rate 136 bytes, 32-byte digest.
//   leaf = Keccak256( le64(canonical(e_0)) || le64(canonical(e_1)) || ... ),   node = Keccak256( left[32] || right[32] )
// lane = leaf / node; the 25-lane state lives in VGPRs (50 registers); a rate block is 17 field elements = 17 state lanes,
// so absorbing is 17 coalesced column loads XORed straight into the state.  Digests: state lanes 0..3 (little endian).
// The per-lane kernel bodies (tree leaves through their three doors, node layers, proof of work) are the plan of byte_tree.h,
// shared with blake2s.hip; the fetches, the launch helpers and the entry this file contributes to the hasher dispatch of
// tree_hash.hip are in tree_plan.h.  Here: the permutation, the policy with the ONE block loop (17 words + pad10*1), the entry points.
#include "gl.h"
#include "kernels.h"
#include "byte_tree.h"
#include "verify_open.h"

using gl::u64;
using gl::u32;

namespace bj {
namespace {

__device__ __constant__ const u64 KECCAK_RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
    0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
    0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
    0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};

template <unsigned N>
__device__ __forceinline__ u64 rotl64(u64 x) {
    if (N == 0) return x;
    return (x << (N & 63)) | (x >> ((64 - N) & 63));
}

// Keccak-f[1600], lanes a[x + 5y]
__device__ __forceinline__ void keccak_f(u64 (&a)[25]) {
#pragma unroll 1
    for (int round = 0; round < 24; round++) {
        u64 c[5], d[5];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rotl64<1>(c[(x + 1) % 5]);
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] ^= d[i % 5];
        // rho + pi: b[y + 5*((2x + 3y) % 5)] = rotl(a[x + 5y], r[x][y])
        u64 b[25];
        b[0] = a[0];
        b[10] = rotl64<1>(a[1]);   b[20] = rotl64<62>(a[2]);  b[5] = rotl64<28>(a[3]);   b[15] = rotl64<27>(a[4]);
        b[16] = rotl64<36>(a[5]);  b[1] = rotl64<44>(a[6]);   b[11] = rotl64<6>(a[7]);   b[21] = rotl64<55>(a[8]);
        b[6] = rotl64<20>(a[9]);   b[7] = rotl64<3>(a[10]);   b[17] = rotl64<10>(a[11]); b[2] = rotl64<43>(a[12]);
        b[12] = rotl64<25>(a[13]); b[22] = rotl64<39>(a[14]); b[23] = rotl64<41>(a[15]); b[8] = rotl64<45>(a[16]);
        b[18] = rotl64<15>(a[17]); b[3] = rotl64<21>(a[18]);  b[13] = rotl64<8>(a[19]);  b[14] = rotl64<18>(a[20]);
        b[24] = rotl64<2>(a[21]);  b[9] = rotl64<61>(a[22]);  b[19] = rotl64<56>(a[23]); b[4] = rotl64<14>(a[24]);
#pragma unroll
        for (int y = 0; y < 25; y += 5)
#pragma unroll
            for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        a[0] ^= KECCAK_RC[round];
    }
}

struct Keccak {
    u64 a[25];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] = 0;
    }
    // pad10*1 of the original Keccak for a message of `lanes_in_last` whole 8-byte words in the final rate block
    __device__ __forceinline__ void pad_and_permute(unsigned lanes_in_last) {
        u64 first = 0x01ULL, last = 0x8000000000000000ULL;
#pragma unroll
        for (int i = 0; i < 17; i++)
            if ((unsigned)i == lanes_in_last) a[i] ^= first;
        a[16] ^= last;
        keccak_f(a);
    }
    __device__ __forceinline__ void digest(u64 (&d)[4]) const {
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = a[k];
    }
};

// the hash policy of byte_tree.h / verify_open.h.  Every index into the state is a constant after unrolling (a run-time index
// would send the 25 lanes to scratch): the tail is selected by k < rem, the padding lane inside pad_and_permute
struct KeccakTree {
    template <typename W>
    static __device__ __forceinline__ void leaf(W word, unsigned n, u64 (&d)[4]) {
        Keccak st;
        st.init();
        unsigned c = 0;
        for (; c + 17 <= n; c += 17) {   // full rate blocks
#pragma unroll
            for (int k = 0; k < 17; k++) st.a[k] ^= gl::canon(word(c + k));
            keccak_f(st.a);
        }
        const unsigned rem = n - c;      // 0..16 words in the last block, then the padding
#pragma unroll
        for (int k = 0; k < 16; k++)
            if ((unsigned)k < rem) st.a[k] ^= gl::canon(word(c + k));
        st.pad_and_permute(rem);
        st.digest(d);
    }
    static __device__ __forceinline__ void node(const u64 (&l)[4], const u64 (&r)[4], u64 (&d)[4]) {
        Keccak st;
        st.init();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            st.a[k] = l[k];
            st.a[4 + k] = r[k];
        }
        st.pad_and_permute(8);   // 64 message bytes = 8 lanes
        st.digest(d);
    }
    // seed = 5 field elements = 40 bytes, so seed || nonce is six lanes of one rate block
    static __device__ __forceinline__ u64 pow_word(const u64 (&seed)[5], u64 nonce) {
        Keccak st;
        st.init();
#pragma unroll
        for (int k = 0; k < 5; k++) st.a[k] = seed[k];
        st.a[5] = nonce;
        st.pad_and_permute(6);   // 48 message bytes = 6 lanes
        return st.a[0];
    }
};

// the plan of byte_tree.h around this hash
__global__ void __launch_bounds__(256)
keccak_leaves_kernel(const u64 *base, size_t col_stride, const u64 *const *col_ptrs, unsigned n_cols, size_t num_leaves,
                     u64 *digests) {
    byte_leaves<KeccakTree>(base, col_stride, col_ptrs, n_cols, num_leaves, digests);
}
__global__ void __launch_bounds__(256)
keccak_leaves_chunked_kernel(const u64 *src0, const u64 *src1, unsigned n_srcs, unsigned log_e, size_t num_leaves,
                             u64 *digests) {
    byte_leaves_chunked<KeccakTree>(src0, src1, n_srcs, log_e, num_leaves, digests);
}
__global__ void __launch_bounds__(256) keccak_nodes_kernel(const u64 *children, u64 *parents, size_t num_parents) {
    byte_nodes<KeccakTree>(children, parents, num_parents);
}
__global__ void __launch_bounds__(256) keccak_pow_kernel(PowSeed seed, unsigned pow_bits, u64 base, u64 count, unsigned long long *result) {
    byte_pow<KeccakTree>(seed, pow_bits, base, count, result);
}

}  // namespace

// bj_verify / bj_verify_batch: one (query, oracle) Merkle chain per lane over every proof of the launch, chain -> (proof, query)
// through the record table (verify_open.h)
__global__ void __launch_bounds__(VERIFY_OPEN_BLOCK) keccak_verify_openings_kernel(VerifyOpenArgs A) { verify_open<verify_chain_bytes<KeccakTree>>(A); }

TreeHasher keccak_tree_hasher() {
    return {tree_leaves<keccak_leaves_kernel>, tree_leaves_chunked<keccak_leaves_chunked_kernel>, tree_nodes<keccak_nodes_kernel>, nullptr,
            tree_verify_openings<keccak_verify_openings_kernel>, tree_pow<keccak_pow_kernel>};
}

}  // namespace bj
