// Stand-alone check of csrc/oracle_value.h (tests/test_oracle_host.py builds it with the address and undefined-behaviour
// sanitizers): the oracle values answer what the prover used to work out at every site.  The two shapes of
// lean_proof_plan_check.cpp on one GPU, LDE 8, cap 16, quotient degree 4:
//   A  2^10 rows, 92 variables, 8 width-4 lookups, one public input;   B  2^12 rows, 60 variables, no lookups, no public input.
// For the four (setup lean?, proof lean?) combinations:
//   - the streaming predicate against the rule the prover and the plan hard-coded: a set is forced through its monomials iff
//     (the setup is lean and it is the set at z) or the proof is lean; otherwise its size alone decides;
//   - Cols at every coset, and the sources of the first and the last opened polynomial of each oracle on the evaluations and on
//     the monomials, against the pointer arithmetic of the prover's former lde_src / mono_src / round-3 ternaries, written out
//     here by hand on made-up base addresses;
//   - the plan's NUM_LDE entries, one per set that is not streamed.
#include "oracle_value.h"
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

using bj::Opened;
using bj::OpenSrc;
typedef uint64_t u64;

static bool same(const OpenSrc &a, const OpenSrc &b) { return a.c0 == b.c0 && a.c1 == b.c1; }

static void check(const char *name, bool lookups, unsigned log_n) {
    bj_circuit ci{};
    ci.log_n = log_n; ci.num_gp_vars = 60; ci.num_vars = lookups ? 92 : 60; ci.num_constant_cols = lookups ? 8 : 7;
    ci.lookup_width = lookups ? 4 : 0; ci.lookup_reps = lookups ? 8 : 0; ci.table_id_col = lookups ? 7 : 0; ci.quotient_degree = 4;
    bj_proof_config cfg{};
    cfg.fri_lde_factor = 8; cfg.cap_size = 16;
    const bj::ProofLayout L = bj::proof_layout(bj::circuit_shape(&ci, &cfg));
    const unsigned pub_col[1] = {3}, pub_row[1] = {5};
    const size_t n_pub = lookups ? 1 : 0;
    const std::vector<bj::OpeningSet> sets = L.opening_sets(pub_col, pub_row, n_pub);
    CHECK(sets.size() == (lookups ? 4u : 2u));   // at z, at z omega, (A) the lookup sums at 0 and the public input's row
    const size_t n = (size_t)1 << log_n, q = 4, N = 8 * n, Ln = 8 * n, Q = q * n;
    const unsigned *w = L.widths;

    // made-up addresses: one block that is never read, every buffer at a place of its own in it
    size_t words = 0;
    auto place = [&words](size_t len) {
        const size_t at = words;
        words += len + 64;
        return at;
    };
    const size_t at_wit_lde = place(w[0] * Ln), at_s2_lde = place(w[1] * Ln), at_q_lde = place(w[2] * N), at_setup_lde = place(w[3] * Ln),
                 at_setup_coset = place(w[3] * n), at_mono = place(w[0] * n), at_mono_s2 = place(w[1] * n), at_Tm = place(2 * Q),
                 at_setup_mono = place(w[3] * n), at_trees = place(4);
    u64 *const mem = (u64 *)std::malloc(words * 8);
    if (!mem) std::abort();
    u64 *const wit_lde = mem + at_wit_lde, *const s2_lde = mem + at_s2_lde, *const q_lde = mem + at_q_lde, *const d_lde = mem + at_setup_lde,
              *const setup_coset = mem + at_setup_coset, *const trees = mem + at_trees;
    const u64 *const mono = mem + at_mono, *const mono_s2 = mem + at_mono_s2, *const Tm = mem + at_Tm, *const d_mono = mem + at_setup_mono;

    for (int combo = 0; combo < 4; combo++) {
        const bool lean_s = combo & 1, lean_p = combo & 2;
        // the values as the prover makes them
        bj::Oracle o[4] = {bj::oracle_of(w[0], n, Ln, !lean_p), bj::oracle_of(w[1], n, Ln, !lean_p), bj::oracle_of(w[2], n, N, true),
                           bj::oracle_of(w[3], n, Ln, !lean_s)};
        o[bj::ORACLE_QUOTIENT].mono_parts = 2, o[bj::ORACLE_QUOTIENT].mono_part_gap = Q;
        o[0].mono = mono, o[0].evals = wit_lde;        // one coset of it when the proof is lean
        o[1].mono = mono_s2, o[1].evals = s2_lde;
        o[2].mono = Tm, o[2].evals = q_lde;
        o[3].mono = d_mono, o[3].evals = lean_s ? setup_coset : d_lde;
        for (int k = 0; k < 4; k++) o[k].tree = trees + k;
        const unsigned resident = bj::resident_mask(o);
        CHECK(resident == bj::resident_mask(lean_s, lean_p));
        CHECK(resident == ((lean_p ? 0u : 3u) | 4u | (lean_s ? 0u : 8u)));
        for (int k = 0; k < 4; k++) CHECK(o[k].leaf_from_evals() == ((resident >> k & 1) != 0) && o[k].width == w[k]);
        CHECK(o[0].eval_words() == w[0] * (lean_p ? n : Ln) && o[1].eval_words() == w[1] * (lean_p ? n : Ln) && o[2].eval_words() == 2 * q * N &&
              o[3].eval_words() == w[3] * (lean_s ? n : Ln));

        // the streaming predicate, against the former on_monomials arguments and the plan's former rule
        size_t not_streamed = 0;
        for (size_t i = 0; i < sets.size(); i++) {
            const bool forced = (lean_s && i == 0) || lean_p;
            CHECK(bj::can_stream(bj::oracle_mask(sets[i].polys), resident) == !forced);
            not_streamed += forced || bj::base_columns(sets[i].polys) >= bj::WS_LARGE_SET;
        }
        CHECK(sets[0].point == bj::OPEN_AT_Z && bj::oracle_mask(sets[0].polys) == 15u);
        CHECK(sets[1].point == bj::OPEN_AT_Z_OMEGA && bj::oracle_mask(sets[1].polys) == 2u && bj::base_columns(sets[1].polys) == 2);
        if (lookups) {
            CHECK(sets[2].point == bj::OPEN_AT_ZERO && bj::oracle_mask(sets[2].polys) == 2u && bj::base_columns(sets[2].polys) == 18);
            CHECK(sets[3].point == bj::OPEN_AT_ROW && bj::oracle_mask(sets[3].polys) == 1u && bj::base_columns(sets[3].polys) == 1);
            CHECK(bj::can_stream(bj::oracle_mask(sets[3].polys), resident) == !lean_p);   // one column, and still through the monomials
        }
        CHECK(not_streamed == (lean_p ? sets.size() : lookups ? 2u : 1u));   // neither lean: the size rule alone (everything at z; 18 lookup-sum columns)

        // the plan asks the same function: one extended numerator per set that is not streamed
        uint32_t sched[1] = {3};
        bj::WorkspaceShape s = bj::workspace_shape(L, 1, false, 1, pub_col, pub_row, n_pub, false, bj::WS_HOST_ABSORBING, false, sched, 1, 1);
        s.lean = lean_s, s.lean_oracles = lean_p;
        CHECK(s.set_oracles.size() == sets.size());
        size_t num_lde = 0, capacity = 0, coset = 0;
        for (const bj::WorkspaceEntry &e : bj::workspace_plan(s).entries) {
            num_lde += e.id == bj::WS_NUM_LDE, capacity += e.id == bj::WS_CAPACITY, coset += e.id == bj::WS_SETUP_COSET;
            if (e.id == bj::WS_WIT_LDE) CHECK(e.words == o[0].eval_words());
            if (e.id == bj::WS_S2_LDE) CHECK(e.words == o[1].eval_words());
            if (e.id == bj::WS_SETUP_COSET) CHECK(e.words == o[3].eval_words());
        }
        CHECK(num_lde == not_streamed && capacity == (lean_p ? 0u : 1u) && coset == (lean_s ? 1u : 0u));

        // Cols at coset c: the round-3 ternaries
        for (size_t c = 0; c < q; c++) {
            const size_t first = c * n;
            const bj::Cols wc = o[0].cols_at(c), sc = o[1].cols_at(c), uc = o[3].cols_at(c);
            CHECK(wc.p == (lean_p ? wit_lde : wit_lde + first) && wc.stride == (lean_p ? n : Ln));
            CHECK(sc.p == (lean_p ? s2_lde : s2_lde + first) && sc.stride == (lean_p ? n : Ln));
            CHECK(uc.p == (lean_s ? setup_coset : d_lde + first) && uc.stride == (lean_s ? n : Ln));
        }
        for (size_t c = 0; c < 8; c++) CHECK(o[2].cols_at(c).p == q_lde + c * n && o[2].cols_at(c).stride == N);

        // sources of the first and the last opened polynomial of each oracle: the former lde_src / mono_src
        const u64 *bases[4] = {wit_lde, s2_lde, q_lde, lean_s ? setup_coset : d_lde};
        const size_t os = lean_p ? n : Ln, strides[4] = {os, os, N, lean_s ? n : Ln};
        const u64 *monos[4] = {mono, mono_s2, nullptr, d_mono};
        for (unsigned k = 0; k < 4; k++) {
            const Opened *first = nullptr, *last = nullptr;
            for (const Opened &p : L.opened)
                if (p.oracle == k) {
                    if (!first) first = &p;
                    last = &p;
                }
            CHECK(first && last && first != last);
            for (const Opened *p : {first, last}) {
                if (!p) continue;
                const u64 *b = bases[k];
                const OpenSrc lde{b + p->col0 * strides[k], p->col1 == bj::NO_COLUMN ? nullptr : b + p->col1 * strides[k]};
                CHECK(same(o[k].eval_src(*p), lde));
                OpenSrc m;
                if (k == bj::ORACLE_QUOTIENT)
                    m = OpenSrc{Tm + (size_t)(p->col0 / 2) * n, Tm + Q + (size_t)(p->col0 / 2) * n};
                else
                    m = OpenSrc{monos[k] + (size_t)p->col0 * n, p->col1 == bj::NO_COLUMN ? nullptr : monos[k] + (size_t)p->col1 * n};
                CHECK(same(o[k].mono_src(*p), m));
                CHECK((p->col1 == bj::NO_COLUMN) == (k == bj::ORACLE_WITNESS || k == bj::ORACLE_SETUP));   // base-field columns there, F_p^2 pairs in stage 2 and the quotient
            }
        }
        // the last chunk of the quotient, spelled out: column 2 (q - 1) of component 0, and its partner Q words on
        const Opened last_chunk = L.opened[L.nz - 1];
        CHECK(last_chunk.oracle == bj::ORACLE_QUOTIENT && last_chunk.col0 == 2 * (q - 1) && last_chunk.col1 == 2 * q - 1);
        CHECK(o[2].mono_src(last_chunk).c0 == Tm + (q - 1) * n && o[2].mono_src(last_chunk).c1 == Tm + Q + (q - 1) * n);
    }
    std::free(mem);
    std::printf("%s: %zu opening sets, widths %u %u %u %u\n", name, sets.size(), w[0], w[1], w[2], w[3]);
}

int main() {
    check("A", true, 10);
    check("B", false, 12);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("oracle values == expected\n");
    return 0;
}
