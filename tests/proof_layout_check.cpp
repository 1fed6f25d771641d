// Stand-alone check of csrc/proof_layout.h (tests/test_proof_layout_host.py builds it with the address and undefined-behaviour
// sanitizers).  Seven circuit shapes written out here; for each the properties a layout must have whatever the shape is: every
// column of every oracle is opened exactly once, the named positions point at the records they name, the sections of a proof
// and the words of a query are contiguous, the public inputs are partitioned by row in first-appearance order.  Then the shape of
// the golden proof, with numbers that come from the fixture through the command line: V Wc nC num_gp_vars lookup_w lookup_reps
// table_id_col q | n_values_at_z n_values_at_0 and the four leaf widths of the fixture's first query.
#include "proof_layout.h"

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

struct Shape {
    const char *name;
    unsigned log_n, V, gp, Wc, nC, w, reps, table_id_col, q, fri_lde, cap;
    std::vector<unsigned> pub_cols, pub_rows;
};

static bj::CircuitShape shape_of(const Shape &S) {
    bj_circuit c{};
    c.log_n = S.log_n; c.num_vars = S.V; c.num_gp_vars = S.gp; c.num_witness_cols = S.Wc; c.num_constant_cols = S.nC;
    c.lookup_width = S.w; c.lookup_reps = S.reps; c.table_id_col = S.table_id_col; c.quotient_degree = S.q;
    bj_proof_config cfg{};
    cfg.fri_lde_factor = S.fri_lde; cfg.cap_size = S.cap;
    return bj::circuit_shape(&c, &cfg);
}

static void check_shape(const Shape &S) {
    std::printf("shape: %s\n", S.name);
    const bj::CircuitShape cs = shape_of(S);
    const bj::ProofLayout L = bj::proof_layout(cs);
    const bool lk = S.reps > 0, tid_var = lk && S.table_id_col == BJ_TABLE_ID_AS_VARIABLE;
    // the shape: the table-id rule, once
    CHECK(cs.tid_var == tid_var && cs.lookup_cps == S.w + (tid_var ? 1u : 0u) && cs.table_id_col == (tid_var ? 0 : S.table_id_col));
    CHECK((1u << cs.log_fri) == S.fri_lde && cs.cap_size == S.cap);
    // counts, from the definitions (prover.rs:251-343): chunks of q columns, one sum per sub-argument and one for the table
    const unsigned chunks = (S.V + S.q - 1) / S.q;
    CHECK(L.has_lookup == lk && L.n_chunks == chunks && L.n_partials == chunks - 1 && L.n_lookup_terms == (lk ? S.reps + 1 : 0));
    CHECK(L.widths[0] == S.V + S.Wc + (lk ? 1 : 0));
    CHECK(L.widths[1] == 2 * chunks + (lk ? 2 * (S.reps + 1) : 0));
    CHECK(L.widths[2] == 2 * S.q);
    CHECK(L.widths[3] == S.V + S.nC + (lk ? S.w + 1 : 0));
    CHECK(L.nz == S.V + S.Wc + S.nC + S.V + chunks + (lk ? 1 + S.reps + 1 + S.w + 1 : 0) + S.q);

    // every column of every oracle exactly once; an F_p^2 polynomial is an adjacent pair
    CHECK(L.opened.size() == L.nz);
    std::vector<std::vector<int>> seen(4);
    for (int o = 0; o < 4; o++) seen[o].assign(L.widths[o], 0);
    for (const bj::Opened &r : L.opened) {
        CHECK(r.oracle < 4);
        if (r.oracle >= 4) continue;
        const bool ext = r.oracle == bj::ORACLE_STAGE2 || r.oracle == bj::ORACLE_QUOTIENT;
        CHECK(r.col0 < L.widths[r.oracle]);
        if (r.col0 < L.widths[r.oracle]) seen[r.oracle][r.col0]++;
        CHECK(ext ? r.col1 == r.col0 + 1 && r.col1 < L.widths[r.oracle] : r.col1 == bj::NO_COLUMN);
        if (ext && r.col1 < L.widths[r.oracle]) seen[r.oracle][r.col1]++;
    }
    for (int o = 0; o < 4; o++)
        for (unsigned c = 0; c < L.widths[o]; c++) CHECK(seen[o][c] == 1);

    // named positions: ascending in the reference's order, each group where its records say
    const unsigned order[] = {L.at_var, L.at_wit, L.at_const, L.at_sigma, L.at_z, L.at_partial, L.at_mult, L.at_a, L.at_b, L.at_table, L.at_chunk, L.nz};
    const unsigned sizes[] = {S.V, S.Wc, S.nC, S.V, 1, chunks - 1, lk ? 1u : 0u, S.reps, lk ? 1u : 0u, lk ? S.w + 1 : 0u, S.q};
    CHECK(order[0] == 0);
    for (int k = 0; k < 11; k++) CHECK(order[k + 1] == order[k] + sizes[k]);
    auto is = [&](unsigned at, unsigned oracle, unsigned col) {
        return at < L.opened.size() && L.opened[at].oracle == oracle && L.opened[at].col0 == col;
    };
    for (unsigned i = 0; i < S.V; i++) CHECK(is(L.at_var + i, bj::ORACLE_WITNESS, L.var(i)) && is(L.at_sigma + i, bj::ORACLE_SETUP, L.sigma(i)));
    for (unsigned i = 0; i < S.Wc; i++) CHECK(is(L.at_wit + i, bj::ORACLE_WITNESS, L.wit(i)));
    for (unsigned i = 0; i < S.nC; i++) CHECK(is(L.at_const + i, bj::ORACLE_SETUP, L.constant(i)));
    CHECK(is(L.at_z, bj::ORACLE_STAGE2, L.z()));
    for (unsigned j = 0; j + 1 < chunks; j++) CHECK(is(L.at_partial + j, bj::ORACLE_STAGE2, L.partial(j)));
    if (lk) {
        CHECK(is(L.at_mult, bj::ORACLE_WITNESS, L.multiplicity()) && L.multiplicity() == L.widths[0] - 1);
        for (unsigned i = 0; i < S.reps; i++) CHECK(is(L.at_a + i, bj::ORACLE_STAGE2, L.lookup_a(i)));
        CHECK(is(L.at_b, bj::ORACLE_STAGE2, L.lookup_b()) && L.lookup_b() == L.widths[1] - 2);
        for (unsigned j = 0; j <= S.w; j++) CHECK(is(L.at_table + j, bj::ORACLE_SETUP, L.table(j)));
        CHECK(L.table(S.w) == L.widths[3] - 1);
        // the lookup columns of the variables: cps per sub-argument behind the general-purpose ones, inside the variables
        CHECK(L.lookup_var(0, 0) == S.gp && L.lookup_var(S.reps - 1, cs.lookup_cps - 1) == S.gp + S.reps * cs.lookup_cps - 1);
        CHECK(L.lookup_var(S.reps - 1, cs.lookup_cps - 1) < S.V);
        if (!tid_var) CHECK(L.table_id() == S.V + S.table_id_col && L.table_id() < L.table(0));
    }
    for (unsigned j = 0; j < S.q; j++) CHECK(is(L.at_chunk + j, bj::ORACLE_QUOTIENT, L.chunk(j)));
    CHECK(L.wit(0) == S.V && L.constant(0) == S.V && L.table(0) == S.V + S.nC);

    // opening sets: z, z * omega, 0 (with lookups), then the public inputs by row
    const size_t n_pub = S.pub_cols.size();
    const std::vector<bj::OpeningSet> sets = L.opening_sets(S.pub_cols.data(), S.pub_rows.data(), n_pub);
    const size_t fixed = lk ? 3 : 2;
    CHECK(sets.size() >= fixed);
    if (sets.size() >= fixed) {
        CHECK(sets[0].point == bj::OPEN_AT_Z && sets[0].polys.size() == L.nz && sets[0].value.size() == L.nz);
        for (unsigned i = 0; i < L.nz && i < sets[0].value.size(); i++) CHECK(sets[0].value[i] == i && sets[0].polys[i].col0 == L.opened[i].col0);
        CHECK(sets[1].point == bj::OPEN_AT_Z_OMEGA && sets[1].polys.size() == 1 && sets[1].polys[0].oracle == bj::ORACLE_STAGE2 &&
              sets[1].polys[0].col0 == L.z() && sets[1].polys[0].col1 == L.z() + 1 && sets[1].value.size() == 1 && sets[1].value[0] == 0);
        if (lk) {
            CHECK(sets[2].point == bj::OPEN_AT_ZERO && sets[2].polys.size() == S.reps + 1 && sets[2].value.size() == S.reps + 1);
            for (unsigned i = 0; i <= S.reps && i < sets[2].polys.size(); i++)
                CHECK(sets[2].polys[i].oracle == bj::ORACLE_STAGE2 && sets[2].polys[i].col0 == L.lookup_a(i) && sets[2].value[i] == i);
        }
    }
    // the public inputs: every input in exactly one set, the set of its row; rows distinct, in first-appearance order; inside a
    // set the inputs in the order given
    std::vector<int> used(n_pub, 0);
    std::vector<unsigned> first_rows;
    for (size_t i = 0; i < n_pub; i++) {
        bool known = false;
        for (unsigned r : first_rows) known = known || r == S.pub_rows[i];
        if (!known) first_rows.push_back(S.pub_rows[i]);
    }
    CHECK(sets.size() == fixed + first_rows.size());
    for (size_t k = fixed; k < sets.size(); k++) {
        const bj::OpeningSet &P = sets[k];
        CHECK(P.point == bj::OPEN_AT_ROW && k - fixed < first_rows.size() && P.row == first_rows[k - fixed]);
        CHECK(!P.polys.empty() && P.polys.size() == P.value.size());
        for (size_t i = 0; i < P.polys.size() && i < P.value.size(); i++) {
            const unsigned v = P.value[i];
            CHECK(v < n_pub);
            if (v >= n_pub) continue;
            used[v]++;
            CHECK(S.pub_rows[v] == P.row && P.polys[i].oracle == bj::ORACLE_WITNESS && P.polys[i].col0 == S.pub_cols[v] && P.polys[i].col1 == bj::NO_COLUMN);
            if (i) CHECK(P.value[i - 1] < v);
        }
    }
    for (size_t i = 0; i < n_pub; i++) CHECK(used[i] == 1);

    // the serialised words under a schedule of every step size: sections and query words contiguous
    const uint32_t sched[3] = {3, 2, 1};
    const size_t sched_len = 3, final_degree = 4, n_queries = 5;
    const bj::SerialLayout A = bj::serial_layout(L, sched, sched_len, final_degree, n_queries, n_pub);
    CHECK(A.ok);
    const unsigned log_full = S.log_n + cs.log_fri;
    unsigned log_cap = 0;
    while ((1u << log_cap) < S.cap) log_cap++;
    CHECK(A.depth == log_full - log_cap);
    const size_t starts[] = {A.header, A.schedule, A.public_inputs, A.witness_cap, A.stage2_cap, A.quotient_cap, A.values_at_z, A.values_at_z_omega,
                             A.values_at_0, A.fri_caps, A.final_c0, A.final_c1, A.queries, A.total};
    const size_t words[] = {19, sched_len, n_pub, 4 * (size_t)S.cap, 4 * (size_t)S.cap, 4 * (size_t)S.cap, 2 * (size_t)L.nz, 2, 2 * (size_t)L.n_lookup_terms,
                            sched_len * 4 * S.cap, final_degree, final_degree, n_queries * A.query_words};
    CHECK(starts[0] == 0);
    for (int k = 0; k < 13; k++) CHECK(starts[k + 1] == starts[k] + words[k]);
    size_t o = 1;   // the index word
    for (int k = 0; k < 4; k++) {
        CHECK(A.leaf_off[k] == o && A.path_off[k] == o + L.widths[k]);
        o += L.widths[k] + 4 * (size_t)A.depth;
    }
    unsigned folded = 0;
    for (size_t l = 0; l < sched_len; l++) {
        folded += sched[l];
        CHECK(A.fri_depth[l] == log_full - folded - log_cap);
        CHECK(A.fri_leaf_off[l] == o && A.fri_path_off[l] == o + ((size_t)2 << sched[l]));
        o += ((size_t)2 << sched[l]) + 4 * (size_t)A.fri_depth[l];
    }
    CHECK(A.query_words == o && A.total_folds == folded);
    // the header: what fill writes, matches accepts, and refuses with any fixed word changed
    bj::ProofHeader H;
    H.fill(L, n_pub, sched_len, final_degree, n_queries, A.depth, 7, 99);
    const uint64_t expected[19] = {0x424A5046ULL, 2, n_pub, S.cap, L.nz, 1, L.n_lookup_terms, sched_len, final_degree, n_queries, L.widths[0], L.widths[1],
                                   L.widths[2], L.widths[3], A.depth, S.log_n, S.fri_lde, 7, 99};
    for (int i = 0; i < 19; i++) CHECK(H.w[i] == expected[i]);
    for (int i = 0; i < 19; i++) {
        uint64_t W[19];
        for (int k = 0; k < 19; k++) W[k] = expected[k];
        W[i] += 1;
        CHECK(H.matches(W) == (i == bj::ProofHeader::N_QUERIES || i == bj::ProofHeader::POW_CHALLENGE));
    }
    // schedules no prover emits, a domain below the cap
    const uint32_t bad_step[1] = {4}, zero_step[1] = {0};
    CHECK(!bj::serial_layout(L, bad_step, 1, 1, 1, 0).ok && !bj::serial_layout(L, zero_step, 1, 1, 1, 0).ok);
    std::vector<uint32_t> deep(32, 3);
    CHECK(!bj::serial_layout(L, deep.data(), deep.size(), 1, 1, 0).ok);   // folds below the cap
    bj::CircuitShape tiny = cs;
    tiny.log_n = 1; tiny.log_fri = 1; tiny.cap_size = 8;
    CHECK(!bj::serial_layout(bj::proof_layout(tiny), sched, 0, 1, 1, 0).ok);
}

int main(int argc, char **argv) {
    const unsigned AS_VAR = BJ_TABLE_ID_AS_VARIABLE;
    const Shape shapes[] = {
        //                                                      log_n  V   gp  Wc nC  w reps tid     q lde cap  public inputs (cols, rows)
        {"no lookups, V not a multiple of q",                    9,    11, 11, 0, 5,  0, 0,  0,      4, 4, 4,   {2}, {5}},
        {"lookups, table id in a constant column",               9,    92, 60, 0, 8,  4, 8,  7,      4, 2, 8,   {3, 10}, {5, 16}},
        {"lookups, table id as a variable (cps = w + 1)",        9,    64, 20, 0, 6,  3, 11, AS_VAR, 4, 2, 4,   {}, {}},
        {"non-copiable witness columns",                         10,   24, 12, 7, 6,  3, 4,  5,      8, 8, 16,  {0}, {0}},
        {"V <= q: no partial products",                          8,    4,  4,  0, 3,  0, 0,  0,      4, 2, 4,   {}, {}},
        {"public inputs: two on one row, that row not first",    9,    29, 20, 2, 8,  4, 2,  7,      4, 4, 4,   {6, 1, 9}, {17, 40, 40}},
        {"public inputs: the shared row split by another",       9,    29, 20, 0, 8,  4, 2,  7,      4, 4, 4,   {6, 1, 9, 2}, {40, 17, 40, 17}},
    };
    for (const Shape &S : shapes) check_shape(S);

    // the golden proof: its counts are the fixture's, not this header's
    if (argc != 15) {
        std::printf("usage: %s V Wc nC num_gp_vars lookup_w lookup_reps table_id_col q n_at_z n_at_0 w_witness w_stage2 w_quotient w_setup\n", argv[0]);
        return 2;
    }
    unsigned a[14];
    for (int i = 0; i < 14; i++) a[i] = (unsigned)std::strtoul(argv[1 + i], nullptr, 10);
    const Shape golden{"golden proof", 20, a[0], a[3], a[1], a[2], a[4], a[5], a[6], a[7], 2, 32, {0, 1, 2, 3}, {7, 7, 7, 7}};
    check_shape(golden);
    const bj::ProofLayout G = bj::proof_layout(shape_of(golden));
    CHECK(G.nz == a[8] && G.n_lookup_terms == a[9]);
    for (int o = 0; o < 4; o++) CHECK(G.widths[o] == a[10 + o]);
    std::printf("golden: nz %u (fixture %u), sums at 0 %u (%u), widths %u %u %u %u (%u %u %u %u)\n", G.nz, a[8], G.n_lookup_terms, a[9], G.widths[0],
                G.widths[1], G.widths[2], G.widths[3], a[10], a[11], a[12], a[13]);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("proof layout == expected\n");
    return 0;
}
