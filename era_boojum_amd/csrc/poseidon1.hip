// Poseidon (v1) (Goldilocks, t = 12, rate 8 / capacity 4, x^7, 4 + 22 + 4 rounds) Merkle-tree hashing for gfx950:
// the tree hasher GoldilocksPoseidonSponge<AbsorptionModeOverwrite> of the reference.
//
// Must equal the reference's CPU tree hasher bit for bit (as canonical residues):
//   permutation        src/implementations/poseidon_goldilocks_naive.rs:67-165
//                      every round: + its 12 constants (the 360-entry table Poseidon2 uses), x^7 on all 12 words (rounds
//                      0-3, 26-29) or on word 0 (rounds 4-25), then the circulant MDS M[row][col] = 2^EXPS[(col - row) mod 12]
//   sponge             src/algebraic_props/sponge.rs:345-357             the Poseidon2 sponge around this permutation
//
// The sponge, the leaf / node hashes, the tree layouts and the mapping (one lane = one leaf or one parent node, the state in
// VGPRs) are the plan of sponge_tree.h, shared with poseidon2.hip; the fetches, the launch helper and the entry this file
// contributes to the hasher dispatch of tree_hash.hip are in tree_plan.h.  Here: the arithmetic, the permutation, the entry points.
// Arithmetic is lazy as in poseidon2.hip: state words are weak residues (any u64 congruent to the value) between rounds;
// the MDS layer's entries are powers of two: the low and the high 32-bit halves of the state are accumulated apart, one
// multiply-add by 2^e per term (no reduction inside the sum), and folded once per output word.
#include "gl.h"
#include "kernels.h"
#include "poseidon1_mds.h"
#include "poseidon_rc.inc"
#include "sponge_tree.h"
#include "verify_open.h"

using gl::u64;
using gl::u32;

namespace bj {

__constant__ u64 POSEIDON1_RC[BJ_POSEIDON_NUM_RC] = BJ_POSEIDON_RC_TABLE;

namespace {

// weak + canonical constant -> weak: "+EPS" on carry; the wrapped sum is < rc < p, so adding EPS cannot carry again
__device__ __forceinline__ u64 p1_add_rc(u64 x, u64 rc) {
    const u64 s = x + rc;
    return s < x ? s + 0xFFFFFFFFull : s;
}
__device__ __forceinline__ u64 p1_pow7(u64 x) {   // weak -> weak
    const u64 x2 = gl::mul_weak(x, x), x3 = gl::mul_weak(x2, x), x4 = gl::mul_weak(x2, x2);
    return gl::mul_weak(x4, x3);
}

__device__ __forceinline__ void p1_full_round(u64 (&s)[12], int r) {
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = p1_pow7(p1_add_rc(s[k], POSEIDON1_RC[12 * r + k]));
    p1_mds(s);
}

}  // namespace

// state in: any u64 words; state out: weak words (canonicalise what leaves the sponge with gl::canon)
__device__ __forceinline__ void poseidon1_permutation(u64 (&s)[12]) {
    int r = 0;
#pragma unroll 1
    for (int i = 0; i < 4; i++, r++) p1_full_round(s, r);
#pragma unroll 1
    for (int i = 0; i < 22; i++, r++) {
        s[0] = p1_pow7(p1_add_rc(s[0], POSEIDON1_RC[12 * r]));
#pragma unroll
        for (int k = 1; k < 12; k++) s[k] = p1_add_rc(s[k], POSEIDON1_RC[12 * r + k]);
        p1_mds(s);
    }
#pragma unroll 1
    for (int i = 0; i < 4; i++, r++) p1_full_round(s, r);
}

// the plan of sponge_tree.h around this permutation (the chunked leaves keep their loop here, as in poseidon2.hip)
__global__ void __launch_bounds__(256)
poseidon1_leaves_kernel(const u64 *base, size_t col_stride, const u64 *const *col_ptrs, unsigned n_cols, size_t num_leaves,
                        u64 *digests) {
    sponge_leaves<poseidon1_permutation>(base, col_stride, col_ptrs, n_cols, num_leaves, digests);
}
__global__ void __launch_bounds__(256)
poseidon1_leaves_absorb_kernel(const u64 *base, size_t col_stride, unsigned n_cols, size_t num_leaves, u64 *capacity, u64 *digests,
                               int first, int last) {
    sponge_leaves_absorb<poseidon1_permutation>(base, col_stride, n_cols, num_leaves, capacity, digests, first, last);
}
__global__ void __launch_bounds__(256)
poseidon1_leaves_chunked_kernel(const u64 *src0, const u64 *src1, unsigned n_srcs, unsigned log_e, size_t num_leaves,
                                u64 *digests) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    const unsigned E = 1u << log_e, total = n_srcs * E;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = 0;
    for (unsigned t = 0; t < total; t += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = t + k < total ? chunk_word(src0, src1, log_e, E, j, t + k) : 0;   // t + k is wave-uniform
        poseidon1_permutation(s);
    }
    sponge_store_digest(digests, j, s);
}
__global__ void __launch_bounds__(256) poseidon1_nodes_kernel(const u64 *children, u64 *parents, size_t num_parents) {
    sponge_nodes<poseidon1_permutation>(children, parents, num_parents);
}
// bj_verify / bj_verify_batch: one (query, oracle) Merkle chain per lane over every proof of the launch, chain -> (proof, query)
// through the record table (verify_open.h)
__global__ void __launch_bounds__(VERIFY_OPEN_BLOCK) poseidon1_verify_openings_kernel(VerifyOpenArgs A) { verify_open<verify_chain_sponge<poseidon1_permutation>>(A); }
__global__ void poseidon1_permute_states_kernel(u64 *states, size_t n_states) { sponge_permute_states<poseidon1_permutation>(states, n_states); }

TreeHasher poseidon1_tree_hasher() {
    return {tree_leaves<poseidon1_leaves_kernel>, tree_leaves_chunked<poseidon1_leaves_chunked_kernel>, tree_nodes<poseidon1_nodes_kernel>,
            tree_leaves_absorb<poseidon1_leaves_absorb_kernel>, tree_verify_openings<poseidon1_verify_openings_kernel>, nullptr};
}

void launch_poseidon1_permute_states(u64 *d_states, size_t n_states, hipStream_t s) {
    hipLaunchKernelGGL(poseidon1_permute_states_kernel, dim3((unsigned)((n_states + 63) / 64)), dim3(64), 0, s, d_states, n_states);
}

}  // namespace bj
