// The hasher-dispatching Merkle-tree entry points of the C ABI and the prover (hasher = BJ_HASHER_*): one table of what the
// hasher files contribute (tree_plan.h), and the walk over the node layers, which is the same for every hasher.
#include "kernels.h"
#include "tree_plan.h"
#include "verify_open.h"
#include "../../include/boojum_hip.h"

namespace bj {

// indexed by BJ_HASHER_*.  The ABI validates the value where it is set; anything else is Poseidon2, the default
static const TreeHasher &tree_hasher(int hasher) {
    static const TreeHasher TABLE[] = {poseidon2_tree_hasher(), poseidon2_tree_hasher(), blake2s_tree_hasher(), keccak_tree_hasher(),
                                       poseidon1_tree_hasher()};
    static_assert(BJ_HASHER_POSEIDON2 == 1 && BJ_HASHER_BLAKE2S == 2 && BJ_HASHER_KECCAK256 == 3 && BJ_HASHER_POSEIDON == 4, "TABLE order");
    return TABLE[hasher > 0 && hasher < (int)(sizeof TABLE / sizeof *TABLE) ? hasher : BJ_HASHER_POSEIDON2];
}

void launch_tree_leaves(int hasher, const u64 *d_base, size_t col_stride, const u64 *const *d_col_ptrs, unsigned n_cols,
                        size_t num_leaves, u64 *d_digests, hipStream_t s) {
    tree_hasher(hasher).leaves(d_base, col_stride, d_col_ptrs, n_cols, num_leaves, d_digests, s);
}
void launch_tree_leaves_chunked(int hasher, const u64 *d_src0, const u64 *d_src1, unsigned n_srcs, unsigned log_e,
                                size_t num_leaves, u64 *d_digests, hipStream_t s) {
    tree_hasher(hasher).leaves_chunked(d_src0, d_src1, n_srcs, log_e, num_leaves, d_digests, s);
}
// tree layout: layer 0 = num_leaves digests, then num_leaves/2, ... down to cap_size (inclusive), back to back
void launch_tree_node_layers(int hasher, u64 *d_tree, size_t num_leaves, size_t cap_size, hipStream_t s) {
    const TreeHasher &h = tree_hasher(hasher);
    u64 *prev = d_tree;
    for (size_t len = num_leaves; len > cap_size; len /= 2) {
        u64 *next = prev + 4 * len;
        h.nodes(prev, next, len / 2, s);
        prev = next;
    }
}
void launch_tree_leaves_absorb(int hasher, const u64 *d_base, size_t col_stride, unsigned n_cols, size_t num_leaves,
                               u64 *d_capacity, u64 *d_digests, bool first, bool last, hipStream_t s) {
    const TreeHasher &h = tree_hasher(hasher);   // callers ask for an algebraic hasher; any other value is Poseidon2, as above
    (h.leaves_absorb ? h : tree_hasher(BJ_HASHER_POSEIDON2)).leaves_absorb(d_base, col_stride, n_cols, num_leaves, d_capacity, d_digests, first, last, s);
}
void launch_verify_openings(int hasher, const VerifyOpenArgs &args, hipStream_t s) { tree_hasher(hasher).verify_openings(args, s); }
// pow_runner = BJ_POW_*; 0 is Blake2s, the reference's default runner
void launch_pow(int pow_runner, const u64 *seed5, unsigned pow_bits, u64 base, u64 count, u64 *d_result, hipStream_t s) {
    PowSeed seed;
    for (int k = 0; k < 5; k++) seed.w[k] = seed5[k];
    tree_hasher(pow_runner == BJ_POW_KECCAK256 ? BJ_HASHER_KECCAK256 : BJ_HASHER_BLAKE2S).pow(seed, pow_bits, base, count, d_result, s);
}

}  // namespace bj
