// bj_verify / bj_verify_batch, the Merkle half of the per-query work (verifier.rs:2150-2232 for the base oracles, :2387-2519 for
// the FRI layers): one chain per (query, oracle) — hash the opened leaf, walk the sibling path with the bits of the leaf's index,
// compare with the cap entry the walk ends at.  The chain bodies here are templates over what each tree hasher brings (the sponge
// permutation of poseidon2.hip / poseidon1.hip, the hash policy of blake2s.hip / keccak.hip); every hasher file wraps
// verify_open around one in a __global__ kernel of its own and adds its launcher to the dispatch of tree_hash.hip.
//
// One launch runs the chains of every proof of a batch under ONE key; bj_verify is the batch of one.  Grid: blockIdx.y = oracle
// (0 witness, 1 stage 2, 2 quotient, 3 setup, 4 + l = FRI layer l), blockIdx.x * 64 + lane = chain of that oracle over the whole
// batch, 64 lanes per workgroup: the lanes of a wave work on ONE oracle, so leaf width and path depth — the number of
// permutations — are wave-uniform; the oracle table is the key's and therefore the batch's.  The (proof, query) a chain belongs to
// comes out of a table of per-proof records in device memory (VerifyBatchProof, ordered by first chain) by a binary search of at
// most 17 steps (none for one record) — a few dozen cached loads in front of ~200 dependent permutations, against a chain ->
// proof array of up to 2^16 x queries words that would have to be built and uploaded per call.  Chains of different proofs share
// waves.  A chain reads its own query's words (a few hundred, uncoalesced: a proof's query section is under 2 MB) and writes one
// status word; nothing here traps, whatever the words are.
#pragma once
#include "gl.h"
#include "verify_batch_plan.h"

namespace bj {
typedef uint64_t u64;

constexpr unsigned VERIFY_MAX_ORACLES = 4 + 32;   // bj_fri_schedule hands out at most 32 steps
constexpr unsigned VERIFY_OPEN_BLOCK = 64;

struct VerifyOracle {
    uint32_t leaf_off;   // words from the start of a query's block to this oracle's leaf elements; the path follows them
    uint32_t width;      // leaf elements
    uint32_t depth;      // path digests (0: the leaf hash is a cap entry)
    uint32_t shift;      // leaf index in this tree = query index >> shift
    uint32_t cap_off;    // words from d_caps to this oracle's cap
};
struct VerifyOpenArgs {
    const u64 *base;                  // the batch's scratch: every offset of a record is in words from here
    const VerifyBatchProof *proofs;   // [n_proofs], chain0 ascending
    uint32_t *status;                 // [n_oracles][n_chains]: 1 = the path leads to the cap, 0 = it does not
    uint32_t n_proofs, n_chains, query_words, n_oracles;
    VerifyOracle oracle[VERIFY_MAX_ORACLES];
};

// the record chain g of a launch belongs to: the last one with chain0 <= g (records without queries never own a chain)
__device__ __forceinline__ unsigned verify_batch_proof_of(const VerifyBatchProof *proofs, unsigned n_proofs, unsigned g) {
    unsigned lo = 0, hi = n_proofs;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (proofs[mid].chain0 <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the algebraic hashers (sponge_tree.h: overwrite absorption of 8 words, zero-padded tail; node = perm(left || right || 0)).
// ONE call site of the permutation serves the leaf's blocks and the path's nodes: which of the two a round is depends on the
// oracle alone, so the branch is wave-uniform (sponge_tree.h: a leaf kernel with two copies of the Poseidon2 stream is 72 KB of
// code; what a second copy would cost HERE was not measured).  Leaf and sibling words enter the sponge as they are, as in
// sponge_leaves / sponge_nodes: the permutation takes any u64 representative, so a word and word + p hash alike, which is what
// the prover's own trees do; the byte hashers hash canonical bytes, as theirs do
template <void (*PERMUTE)(u64 (&)[12])>
__device__ __forceinline__ bool verify_chain_sponge(const u64 *query, u64 index, const VerifyOracle &O, const u64 *caps) {
    const u64 *leaf = query + O.leaf_off, *path = leaf + O.width;
    u64 ti = index >> O.shift;
    const unsigned n_blocks = (O.width + 7) / 8, rounds = n_blocks + O.depth;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = 0;
    for (unsigned r = 0; r < rounds; r++) {
        if (r < n_blocks) {
#pragma unroll
            for (int k = 0; k < 8; k++) s[k] = 8 * r + k < O.width ? leaf[8 * r + k] : 0;
        } else {
            const u64 *sib = path + 4 * (r - n_blocks);
            const bool right = ti & 1;   // this node is the right child: the sibling goes first
            ti >>= 1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u64 d = gl::canon(s[k]), b = sib[k];
                s[k] = right ? b : d;
                s[4 + k] = right ? d : b;
            }
#pragma unroll
            for (int k = 8; k < 12; k++) s[k] = 0;
        }
        PERMUTE(s);
    }
    const u64 *cap = caps + O.cap_off + 4 * ti;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) ok = ok && gl::canon(s[k]) == cap[k];
    return ok;
}

// the byte hashers (the policy of byte_tree.h): H::leaf(word, n, digest) hashes the canonical little-endian bytes of the n field
// elements word(0..n), H::node(l, r, digest) the 64 bytes of two digests; digests are four raw words
template <typename H>
__device__ __forceinline__ bool verify_chain_bytes(const u64 *query, u64 index, const VerifyOracle &O, const u64 *caps) {
    const u64 *leaf = query + O.leaf_off, *path = leaf + O.width;
    u64 ti = index >> O.shift;
    u64 d[4];
    H::leaf([=](unsigned c) { return leaf[c]; }, O.width, d);
    for (unsigned j = 0; j < O.depth; j++) {
        const u64 *sib = path + 4 * j;
        const bool right = ti & 1;
        ti >>= 1;
        u64 l[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            l[k] = right ? sib[k] : d[k];
            r[k] = right ? d[k] : sib[k];
        }
        H::node(l, r, d);
    }
    const u64 *cap = caps + O.cap_off + 4 * ti;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) ok = ok && d[k] == cap[k];
    return ok;
}

// one chain of a launch: which (proof, query) it belongs to, the chain body CHAIN (verify_chain_sponge<PERMUTE> or
// verify_chain_bytes<H>), its status word
template <bool (*CHAIN)(const u64 *, u64, const VerifyOracle &, const u64 *)>
__device__ __forceinline__ void verify_open(const VerifyOpenArgs &A) {
    const unsigned g = blockIdx.x * VERIFY_OPEN_BLOCK + threadIdx.x, o = blockIdx.y;
    if (g >= A.n_chains) return;
    const VerifyBatchProof &P = A.proofs[verify_batch_proof_of(A.proofs, A.n_proofs, g)];
    const unsigned c = g - P.chain0;
    if (c >= P.nq) return;
    // query base, cap base and index are per-lane values (a wave may span proofs): nothing else of the record stays live
    const u64 *query = A.base + P.queries + (size_t)c * A.query_words, *caps = A.base + P.caps;
    const u64 index = A.base[P.indices + c];
    const bool ok = CHAIN(query, index, A.oracle[o], caps);
    A.status[(size_t)o * A.n_chains + g] = ok ? 1u : 0u;
}

}  // namespace bj
