// Stand-alone check of csrc/workspace_plan.h (tests/test_workspace_plan_host.py builds it with the address and undefined-behaviour
// sanitizers).  Shapes: 2^8, 2^12, 2^16, 2^22 (tiled monomials) and 2^23 rows; one, two and eight ranks; with and without lookups;
// multiplicities supplied or counted into the arena; the three host-witness modes; zero, one and three public-input rows; proof of
// work on and off.  For each: every entry starts on a multiple of 64 words behind the previous one and total() is the end of the
// last; the exact entries are the ones that path takes, in the order it takes them (written out here a second time, as
// conditions); total() does not exceed the 13-term sum that reserved the workspace before there was a plan.  The bench's circuit
// at 2^22 rows on one GPU must come to the high-water mark DESIGN.md §6 records (62.4 GB).
#include "workspace_plan.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

struct Case {
    unsigned log_n, world;
    bool lookups, count_mult;
    unsigned host_witness;
    std::vector<unsigned> pub_cols, pub_rows;
    unsigned pow_bits;
};

// compute_fri_schedule (prover.rs:2281-2372) as bj_fri_schedule states it
static void schedule(unsigned security, size_t cap, unsigned pow_bits, unsigned rate_log2, unsigned deg, uint32_t *sched, size_t *len,
                     size_t *num_queries, unsigned *new_pow) {
    auto log2_of = [](size_t x) {
        unsigned r = 0;
        while (((size_t)1 << r) < x) r++;
        return r;
    };
    unsigned raw = security - pow_bits;
    *new_pow = pow_bits;
    if (raw % rate_log2 != 0 && *new_pow >= rate_log2 - raw % rate_log2) *new_pow -= rate_log2 - raw % rate_log2;
    raw = security - *new_pow;
    *num_queries = raw / rate_log2 + (raw % rate_log2 != 0 ? 1 : 0);
    const unsigned stop_log = log2_of(cap >> rate_log2 ? cap >> rate_log2 : 1), cap_log = log2_of(cap);
    *len = 0;
    while (deg > stop_log) {
        if (deg + rate_log2 <= cap_log) break;
        const unsigned gap = deg - stop_log, k = gap >= 3 ? 3 : gap;
        deg -= k;
        sched[(*len)++] = k;
        if ((k == 1 && gap == 1) || deg + rate_log2 <= cap_log) break;
    }
}

// The reservation before the plan: the sum prover.hip held, "sizes mirror the allocations", its fudge terms included.
static size_t parent_formula(const bj::WorkspaceShape &s, size_t n_pub, size_t n_chunks) {
    const size_t slack = (size_t)1 << 17, n = s.n, N = s.N, Ln = s.Ln, Q = s.Q, W = s.world, tree = s.tree_words;
    return (size_t)s.nW * Ln + (size_t)(s.nW + s.nS2) * n + tree + (size_t)s.nS2 * n + ((size_t)2 * n_chunks * n + 2 * ((n + 1023) / 1024) + 16) +
           (size_t)s.nS2 * Ln + tree + 2 * Q + (W > 1 ? 2 * Ln * (W + 1) : 0) + (size_t)2 * s.q * N + tree + 4 * n + 4 * N +
           (size_t)4096 * 1024 * (W > 1 ? 1 + W : 1) + 64 * slack + 4 * N + (N * W) / 2 + (W > 1 ? 10 * n : 0) + 4 * N + (size_t)2 * N * (1 + n_pub) +
           (s.tiled ? 2 * Q : 0) + (s.mult_in_arena ? n + slack : 0);
}

static bj::WorkspaceShape shape_of(const Case &c, bj::ProofLayout *layout) {
    // the bench's SHA-256 geometry (60 general-purpose columns, 8 width-4 lookups, quotient degree 4), LDE 8, cap 16, 100 bits
    bj_circuit ci{};
    ci.log_n = c.log_n; ci.num_gp_vars = 60; ci.num_vars = c.lookups ? 92 : 60; ci.num_constant_cols = c.lookups ? 8 : 7;
    ci.lookup_width = c.lookups ? 4 : 0; ci.lookup_reps = c.lookups ? 8 : 0; ci.table_id_col = c.lookups ? 7 : 0; ci.quotient_degree = 4;
    bj_proof_config cfg{};
    cfg.fri_lde_factor = 8; cfg.cap_size = 16;
    *layout = bj::proof_layout(bj::circuit_shape(&ci, &cfg));
    uint32_t sched[32];
    size_t len = 0, nq = 0;
    unsigned new_pow = 0;
    schedule(100, 16, c.pow_bits, 3, c.log_n, sched, &len, &nq, &new_pow);
    const unsigned alpha_terms = layout->n_lookup_terms + 9 + 1 + layout->n_chunks;
    return bj::workspace_shape(*layout, c.world, c.log_n == 22, alpha_terms, c.pub_cols.data(), c.pub_rows.data(), c.pub_cols.size(),
                               c.lookups && c.count_mult && c.host_witness == bj::WS_HOST_NONE, c.host_witness, new_pow != 0, sched, len, nq);
}

static size_t check_case(const Case &c) {
    bj::ProofLayout L;
    const bj::WorkspaceShape s = shape_of(c, &L);
    const bj::WorkspacePlan P = bj::workspace_plan(s);
    const bool sharded = c.world > 1;
    // alignment; total() is the end of the last entry
    size_t end = 0, exact_words = 0;
    for (const bj::WorkspaceEntry &e : P.entries) {
        CHECK(e.offset % bj::WS_ALIGN == 0 && e.offset >= end && e.offset < end + bj::WS_ALIGN && e.words > 0);
        end = e.offset + e.words;
        if (e.exact) exact_words += e.words;
    }
    CHECK(P.total() == end);
    // the exact entries of this path, in order
    std::vector<bj::WsId> want;
    if (s.mult_in_arena) want.push_back(bj::WS_MULTIPLICITY);
    want.insert(want.end(), {bj::WS_WIT_LDE, bj::WS_MONO, bj::WS_MONO_S2, bj::WS_WIT_TREE});
    if (c.host_witness == bj::WS_HOST_ABSORBING) want.push_back(bj::WS_CAPACITY);
    want.insert(want.end(), {bj::WS_S2_NAT, bj::WS_S2_SCRATCH, bj::WS_S2_LDE, bj::WS_S2_TREE, bj::WS_ALPHAS, bj::WS_T});
    if (sharded) want.insert(want.end(), {bj::WS_T_LOCAL, bj::WS_RESIDUES});
    if (c.log_n == 22) want.push_back(bj::WS_T_TILED);
    want.insert(want.end(), {bj::WS_Q_LDE, bj::WS_Q_TREE, bj::WS_BARY_W, bj::WS_DEEP, bj::WS_NUM_MONO});
    if (sharded) want.push_back(bj::WS_NUM_SLICE);
    want.push_back(bj::WS_NUM_LDE);   // everything at z: more than 16 columns.  The lookup sums at 0: 2 * 9 columns
    if (c.lookups) want.push_back(bj::WS_NUM_LDE);
    for (size_t step = 0; step < s.sched_len; step++) {
        want.insert(want.end(), {bj::WS_FRI_TREE, bj::WS_FRI_LAYER});
        if (sharded && step == 0) want.push_back(bj::WS_FRI_PART);
    }
    want.push_back(bj::WS_FRI_FINAL);
    if (s.pow) want.push_back(bj::WS_POW);
    want.insert(want.end(), {bj::WS_QUERY_IDX, bj::WS_QUERY_BLOCK});
    if (sharded) want.push_back(bj::WS_QUERY_ALL);
    want.insert(want.end(), {bj::WS_FRI_QUERY_IDX, bj::WS_FRI_QUERY_BLOCK});
    size_t k = 0;
    bool staging = false;
    for (const bj::WorkspaceEntry &e : P.entries) {
        if (!e.exact) {
            staging = staging || e.id == bj::WS_GATHER_STAGING;
            continue;
        }
        CHECK(k < want.size() && e.id == want[k]);
        k++;
    }
    CHECK(k == want.size());
    CHECK(staging == sharded);   // one device alone stages no gather
    CHECK(s.pub_set_cols.size() == (c.pub_rows.empty() ? 0u : c.pub_rows.size() == 1 ? 1u : 2u));   // the three-input case shares a row
    // a few sizes from the definitions, not from the plan's own expressions
    const size_t n = (size_t)1 << c.log_n;
    for (const bj::WorkspaceEntry &e : P.entries) {
        if (e.id == bj::WS_WIT_LDE) CHECK(e.words == (size_t)L.widths[0] * n * 8 / c.world);
        if (e.id == bj::WS_Q_LDE) CHECK(e.words == (size_t)8 * n * 8 / c.world);
        if (e.id == bj::WS_CAPACITY) CHECK(e.words == 4 * n * 8 / c.world);
        if (e.id == bj::WS_WIT_TREE) CHECK(e.words == (2 * n * 8 - 16) / c.world * 4);
    }
    // never looser than the sum it replaces
    const size_t parent = parent_formula(s, c.pub_cols.size(), L.n_chunks);
    CHECK(P.total() <= parent);
    std::printf("log_n %2u W %u lookups %d counted %d host %u pub %zu pow %2u: %3zu entries, total %zu words (%.3f GB), allowances %zu, before %zu\n",
                c.log_n, c.world, (int)c.lookups, (int)c.count_mult, c.host_witness, c.pub_cols.size(), c.pow_bits, P.entries.size(), P.total(),
                P.total() * 8e-9, P.allowance_words(), parent);
    return exact_words;
}

int main() {
    const std::vector<unsigned> none, one_col = {3}, one_row = {5}, three_cols = {6, 1, 9}, three_rows = {17, 40, 40};
    for (unsigned log_n : {8u, 12u, 16u, 22u, 23u})
        for (unsigned world : {1u, 2u, 8u})
            for (int variant = 0; variant < 8; variant++) {
                Case c{log_n, world, true, false, bj::WS_HOST_NONE, none, none, 0};
                if (variant == 1) c.lookups = false;
                if (variant == 2) c.count_mult = true;
                if (variant == 3) c.host_witness = bj::WS_HOST_ABSORBING;
                if (variant == 4) c.host_witness = bj::WS_HOST_NOT_ABSORBING, c.count_mult = true;
                if (variant == 5) c.pub_cols = one_col, c.pub_rows = one_row;
                if (variant == 6) c.pub_cols = three_cols, c.pub_rows = three_rows, c.pow_bits = 20;
                if (variant == 7) c.pow_bits = 10, c.host_witness = bj::WS_HOST_ABSORBING, c.lookups = false;
                check_case(c);
            }
    // DESIGN.md §6, W = 1 at 2^22 rows with a resident witness: 62.4 GB at the high-water mark, before every context began to
    // reserve the capacity words (which a resident witness does not take: they are absent from this plan).  On one GPU every
    // allowance is the size the callee takes, so the plan's total is the mark itself.
    {
        const Case bench{22, 1, true, false, bj::WS_HOST_NONE, none, none, 0};
        bj::ProofLayout L;
        const bj::WorkspacePlan P = bj::workspace_plan(shape_of(bench, &L));
        const double exact_gb = check_case(bench) * 8e-9, total_gb = P.total() * 8e-9, allow_gb = P.allowance_words() * 8e-9;
        std::printf("bench shape: exact entries %.3f GB, total %.3f GB, allowances %.6f GB\n", exact_gb, total_gb, allow_gb);
        CHECK(total_gb >= 62.35 && total_gb < 62.45);
        CHECK(total_gb - exact_gb <= allow_gb + 64 * 8e-9 * P.entries.size());
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("workspace plan == expected\n");
    return 0;
}
