// The workspace of a proof, defined once: every buffer a proof takes out of the context's bump-allocated arena, in the order it
// takes them, as a value made from a few numbers that prove_impl knows before its first kernel.  The reservation is the plan's
// total; the prover takes its buffers from the plan by name (TmpBuf::take, ctx.h), so a buffer the plan does not hold, holds
// elsewhere or holds with another size ends the proof with an internal error instead of a hipMalloc in the middle of it.
// Plain C++17, no HIP: a host program can use it (tests/workspace_plan_check.cpp).
#pragma once
#include "callee_words.h"
#include "oracle_value.h"
#include "proof_layout.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bj {

enum WsId : unsigned {
    // exact entries: the buffers the prover takes itself, in the order of the rounds
    WS_MULTIPLICITY, WS_WIT_LDE, WS_MONO, WS_MONO_S2, WS_WIT_TREE, WS_CAPACITY,
    WS_S2_NAT, WS_S2_SCRATCH, WS_S2_LDE, WS_S2_TREE,
    WS_ALPHAS, WS_T, WS_T_LOCAL, WS_RESIDUES, WS_SETUP_COSET, WS_T_TILED, WS_Q_LDE, WS_Q_TREE,
    WS_BARY_W,
    WS_DEEP, WS_NUM_MONO, WS_NUM_SLICE, WS_NUM_LDE,
    WS_FRI_TREE, WS_FRI_LAYER, WS_FRI_PART, WS_FRI_FINAL,
    WS_POW,
    WS_QUERY_IDX, WS_QUERY_BLOCK, WS_QUERY_ALL, WS_FRI_QUERY_IDX, WS_FRI_QUERY_BLOCK,
    // allowances: upper bounds for temporaries that a callee takes (callee_words.h)
    WS_ARGS_EVAL, WS_ARGS_COMBINE, WS_ARGS_DEEP, WS_GATHER_STAGING,
    WS_N_IDS
};
inline const char *ws_name(unsigned id) {
    static const char *const names[WS_N_IDS] = {
        "multiplicity column", "wit_lde", "mono", "mono_s2", "wit_tree", "capacity words",
        "s2_nat", "stage-2 scratch", "s2_lde", "s2_tree",
        "alphas", "T", "T of this rank", "residue gather", "setup coset", "tiled T", "q_lde", "q_tree",
        "barycentric w",
        "deep", "num_mono", "num_slice", "num_lde",
        "FRI tree", "FRI layer", "FRI part", "FRI final buffer",
        "PoW result",
        "query indices", "query block", "gathered query blocks", "FRI query indices", "FRI query blocks",
        "evaluation arguments", "combination arguments", "DEEP arguments", "column gather staging"};
    return id < WS_N_IDS ? names[id] : "?";
}

enum : unsigned { WS_HOST_NONE = 0, WS_HOST_ABSORBING = 1, WS_HOST_NOT_ABSORBING = 2 };
constexpr unsigned WS_LARGE_SET = 16;   // an opening set of this many base columns is combined on its monomials and extended (num_lde)
constexpr size_t WS_ALIGN = 64;         // every entry starts on a multiple of 64 words (512 bytes), as arena_alloc places it

// The numbers the sizes depend on.  N, Ln, Qe, tree_words: of THIS rank (the whole domain on one GPU).
struct WorkspaceShape {
    size_t n = 0, N = 0, Ln = 0, Q = 0, Qe = 0;
    unsigned q = 0;
    unsigned nW = 0, nS2 = 0, n_setup = 0;   // leaf widths of the witness, stage-2 and setup oracles (the quotient's is 2 q)
    unsigned n_chunks = 0;
    unsigned alpha_terms = 0;                // powers of the quotient challenge
    unsigned world = 1;
    bool tiled = false;
    // the residency bits (oracle_value.h: resident_mask), set by the prover, single device only.  lean: the setup's oracle keeps no
    // evaluations (bj_setup::lean); lean_oracles: nor do the witness and stage-2 oracles (BJ_PROOF_LEAN)
    bool lean = false, lean_oracles = false;
    size_t tree_words = 0;                   // bj_merkle_tree_digests(N, cap_size / world) * 4
    unsigned depth = 0;                      // path length of the base oracles: log2(N * world / cap_size)
    unsigned opened_cols = 0;                // base columns of the polynomials opened at z (an F_p^2 polynomial counts two)
    unsigned lookup_terms = 0;               // lookup sums opened at 0 (A_i and B), each an F_p^2 polynomial
    std::vector<unsigned> pub_set_cols;      // one per public-input opening set (row): its columns
    std::vector<unsigned> set_oracles;       // one per opening set, in challenge order: the oracles its polynomials belong to (oracle_mask)
    bool has_lookup = false;
    bool mult_in_arena = false;              // the multiplicity column is counted into a column of the arena
    unsigned host_witness = WS_HOST_NONE;
    bool pow = false;
    uint32_t sched[32] = {};                 // bj_fri_schedule
    size_t sched_len = 0, num_queries = 0, cap_size = 0;
    // a proof from a WitnessVec's values (bj_prove_values): the length of all_values; 0 for every other witness source.  The arena
    // does not depend on it: the values wait in the witness staging (async_admission.h: lane_extras)
    size_t n_values = 0;
};

// The shape of a proof of layout L split over `world` ranks (1: one GPU).  tiled: the monomials' layout (2^22-row traces);
// alpha_terms: powers of the quotient challenge; sched, num_queries: bj_fri_schedule of the proof config; pow: its new_pow_bits != 0.
inline WorkspaceShape workspace_shape(const ProofLayout &L, unsigned world, bool tiled, unsigned alpha_terms, const unsigned *pub_cols,
                                      const unsigned *pub_rows, size_t n_pub, bool mult_in_arena, unsigned host_witness, bool pow,
                                      const uint32_t *sched, size_t sched_len, size_t num_queries) {
    WorkspaceShape w;
    const size_t fri_lde = (size_t)1 << L.s.log_fri, lde = fri_lde > L.s.q ? fri_lde : L.s.q;   // used_lde_degree (prover.rs:313)
    w.n = (size_t)1 << L.s.log_n, w.q = L.s.q, w.world = world, w.tiled = tiled;
    w.N = w.n * fri_lde / world, w.Ln = lde / world * w.n, w.Q = w.n * L.s.q, w.Qe = w.Q / world;
    w.nW = L.widths[ORACLE_WITNESS], w.nS2 = L.widths[ORACLE_STAGE2], w.n_setup = L.widths[ORACLE_SETUP];
    w.n_chunks = L.n_chunks, w.alpha_terms = alpha_terms;
    w.cap_size = L.s.cap_size;
    w.tree_words = (2 * w.N - w.cap_size / world) * 4;   // bj_merkle_tree_digests of the local subtree
    while (((size_t)1 << w.depth) < w.N * world / w.cap_size) w.depth++;
    w.opened_cols = base_columns(L.opened);
    w.has_lookup = L.has_lookup, w.lookup_terms = L.n_lookup_terms;
    for (const OpeningSet &set : L.opening_sets(pub_cols, pub_rows, n_pub)) {
        w.set_oracles.push_back(oracle_mask(set.polys));
        if (set.point == OPEN_AT_ROW) w.pub_set_cols.push_back((unsigned)set.polys.size());
    }
    w.mult_in_arena = mult_in_arena, w.host_witness = host_witness, w.pow = pow;
    for (size_t i = 0; i < sched_len && i < 32; i++) w.sched[i] = sched[i];
    w.sched_len = sched_len < 32 ? sched_len : 32, w.num_queries = num_queries;
    return w;
}

struct WorkspaceEntry {
    WsId id;
    size_t words;
    bool exact;      // false: an allowance
    size_t offset;   // words from the start of the workspace when every allowance is used in full
};

struct WorkspacePlan {
    std::vector<WorkspaceEntry> entries;
    size_t total() const { return entries.empty() ? 0 : entries.back().offset + entries.back().words; }
    size_t allowance_words() const {
        size_t s = 0;
        for (const WorkspaceEntry &e : entries)
            if (!e.exact) s += e.words;
        return s;
    }
    void add(WsId id, size_t words, bool exact) {
        if (exact && !words) words = 1;   // a taken buffer has an address of its own
        entries.push_back({id, words, exact, (total() + WS_ALIGN - 1) & ~(WS_ALIGN - 1)});
    }
    void take(WsId id, size_t words) { add(id, words, true); }
    void allow(WsId id, size_t words) {
        if (words) add(id, words, false);
    }
};

inline WorkspacePlan workspace_plan(const WorkspaceShape &s) {
    WorkspacePlan P;
    const unsigned W = s.world;
    const bool sharded = W > 1;
    auto log2_of = [](size_t x) {
        unsigned r = 0;
        while (((size_t)1 << r) < x) r++;
        return r;
    };
    // round 1: witness
    if (s.mult_in_arena) P.take(WS_MULTIPLICITY, s.n);
    const unsigned resident = resident_mask(s.lean, s.lean_oracles);
    auto is_resident = [resident](unsigned oracle) { return (resident >> oracle & 1) != 0; };
    P.take(WS_WIT_LDE, oracle_of(s.nW, s.n, s.Ln, is_resident(ORACLE_WITNESS)).eval_words());
    P.take(WS_MONO, (size_t)s.nW * s.n);
    P.take(WS_MONO_S2, (size_t)s.nS2 * s.n);
    P.take(WS_WIT_TREE, s.tree_words);
    if (s.host_witness == WS_HOST_ABSORBING && is_resident(ORACLE_WITNESS)) P.take(WS_CAPACITY, 4 * s.N);   // a lean oracle is hashed coset by coset, never group by group
    // round 2: stage 2
    P.take(WS_S2_NAT, (size_t)s.nS2 * s.n);
    P.take(WS_S2_SCRATCH, copy_perm_stage2_scratch_words(s.n_chunks, s.n));
    P.take(WS_S2_LDE, oracle_of(s.nS2, s.n, s.Ln, is_resident(ORACLE_STAGE2)).eval_words());
    P.take(WS_S2_TREE, s.tree_words);
    // round 3: quotient
    P.take(WS_ALPHAS, 2 * (size_t)s.alpha_terms);
    P.take(WS_T, 2 * s.Q);
    if (sharded) {
        P.take(WS_T_LOCAL, 2 * s.Qe);
        P.take(WS_RESIDUES, 2 * s.Q);
    }
    if (!is_resident(ORACLE_SETUP)) P.take(WS_SETUP_COSET, oracle_of(s.n_setup, s.n, s.Ln, false).eval_words());   // one coset of the setup columns at a time; round 4 reads the last one left in it
    if (s.tiled) P.take(WS_T_TILED, 2 * s.Q);
    P.take(WS_Q_LDE, (size_t)2 * s.q * s.N);
    P.take(WS_Q_TREE, s.tree_words);
    // round 4: openings at z, z * omega and (lookup sums) 0.  Sharded, a rank may evaluate a slice of the columns: never more
    P.take(WS_BARY_W, 2 * s.n);
    P.allow(WS_ARGS_EVAL, barycentric_arg_words(s.opened_cols, s.n));
    P.allow(WS_ARGS_EVAL, barycentric_arg_words(2, s.n));
    if (s.has_lookup) P.allow(WS_ARGS_EVAL, barycentric_arg_words(2 * (size_t)s.lookup_terms, s.n));
    // round 5a: DEEP.  The sets in challenge order; a large one leaves an extended numerator (two columns) for the division
    P.take(WS_DEEP, 2 * s.N);
    P.take(WS_NUM_MONO, 2 * s.n);
    if (sharded) P.take(WS_NUM_SLICE, 2 * s.n / W + 16);
    std::vector<size_t> sets = {s.opened_cols, 2};
    if (s.has_lookup) sets.push_back(2 * (size_t)s.lookup_terms);
    sets.insert(sets.end(), s.pub_set_cols.begin(), s.pub_set_cols.end());
    for (size_t i = 0; i < sets.size(); i++) {
        size_t &cols = sets[i];
        if (cols < WS_LARGE_SET && can_stream(s.set_oracles[i], resident)) continue;   // a handful of columns, all of them on the FRI domain
        P.take(WS_NUM_LDE, 2 * s.N);
        P.allow(WS_ARGS_COMBINE, column_list_arg_words(cols));
        if (sharded && s.n % W == 0 && s.n / W >= 256) P.allow(WS_GATHER_STAGING, gather_columns_staging_words(W, 2, s.n / W));
        cols = 2;
    }
    for (size_t i = 0; i < sets.size(); i += DEEP_MAX_SETS) {
        size_t cols = 0;
        for (size_t k = i; k < sets.size() && k < i + DEEP_MAX_SETS; k++) cols += sets[k];
        P.allow(WS_ARGS_DEEP, column_list_arg_words(cols));
    }
    // round 5b: FRI.  Oracle 0 of a sharded proof is committed and folded shard-wise, its folded layer gathered
    size_t len = s.N * W, max_out = 0;
    for (size_t step = 0; step < s.sched_len; step++) {
        const unsigned k = s.sched[step], parts = step == 0 ? W : 1;
        const size_t leaves = (len / parts) >> k, cap = s.cap_size / parts;
        P.take(WS_FRI_TREE, 2 * leaves > cap ? (2 * leaves - cap) * 4 : 0);
        P.take(WS_FRI_LAYER, 2 * (len >> k));
        if (parts > 1) {
            P.take(WS_FRI_PART, 2 * leaves);
            P.allow(WS_GATHER_STAGING, gather_columns_staging_words(W, 2, leaves));
        }
        const size_t out = ((size_t)2 << k) + (size_t)(cap ? log2_of(leaves / cap) : 0) * 4;   // a queried leaf and its path
        if (out > max_out) max_out = out;
        len >>= k;
    }
    P.take(WS_FRI_FINAL, 2 * len);
    if (s.pow) P.take(WS_POW, 8);
    // round 6: queries
    const size_t block = ((size_t)s.nW + s.nS2 + 2 * s.q + s.n_setup + (size_t)4 * s.depth * 4) * s.num_queries;
    P.take(WS_QUERY_IDX, s.num_queries);
    P.take(WS_QUERY_BLOCK, block);
    if (sharded) P.take(WS_QUERY_ALL, block * W);
    P.take(WS_FRI_QUERY_IDX, s.num_queries);
    P.take(WS_FRI_QUERY_BLOCK, max_out * s.num_queries * (W + 1));
    return P;
}

}  // namespace bj
