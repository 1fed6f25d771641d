// Stand-alone host check of csrc/verify_batch_plan.h, built with -fsanitize=address,undefined by tests/test_verify_batch_host.py:
// the scratch of a batch is ONE heap block of exactly total_words words, and everything bj_verify_batch and its two kernels do
// with the plan's offsets is replayed on it — the uploads, the chain -> (proof, query) search of every chain, the reads a chain
// makes at the far end of its blocks, the status words — so that an offset past the block, an overlap of two regions or a chain
// mapped to the wrong proof ends the program.  Prints "ok <cases>" and returns 0 otherwise.
#include "../era_boojum_amd/csrc/verify_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static void claim(std::vector<unsigned char> &owner, size_t at, size_t words, unsigned char tag) {
    CHECK(at + words <= owner.size());
    for (size_t i = 0; i < words; i++) {
        CHECK(owner[at + i] == 0);   // no word belongs to two regions
        owner[at + i] = tag;
    }
}

static void run_pass(const VerifyBatchGeometry &G, const std::vector<VerifyBatchProof> &rec, uint32_t n_chains, uint64_t *D, size_t total,
                     size_t status_open, size_t status_deep, const std::vector<size_t> &expect_proof) {
    uint32_t *st_open = (uint32_t *)(D + status_open), *st_deep = (uint32_t *)(D + status_deep);
    uint32_t g = 0;
    for (size_t p = 0; p < rec.size(); p++)
        for (uint32_t c = 0; c < rec[p].nq; c++, g++) {
            const size_t found = verify_batch_proof_of_host(rec.data(), rec.size(), g);
            CHECK(found == p && found == expect_proof[g]);
            const VerifyBatchProof &R = rec[found];
            CHECK(g - R.chain0 == c && c < R.nq);
            const uint64_t *Q = D + R.queries + (size_t)c * G.query_words;
            CHECK(Q + G.query_words <= D + total);
            uint64_t sum = Q[0] + Q[G.query_words - 1] + D[R.indices + c];            // first and last word of the query's block
            sum += D[R.caps + G.n_oracles * G.cap_words - 1] + D[R.terms + G.term_words - 1] + D[R.sets + G.set_words - 1];
            sum += D[R.fri_ch + G.fri_words - 1] + D[R.final0 + G.final_degree - 1] + D[R.final1 + G.final_degree - 1];
            for (size_t o = 0; o < G.n_oracles; o++) st_open[o * (size_t)n_chains + g] = 1u + (uint32_t)(sum & 1);
            st_deep[g] = (uint32_t)found;
        }
    CHECK(g == n_chains);
    for (size_t p = 0; p < rec.size(); p++)
        for (uint32_t c = 0; c < rec[p].nq; c++) CHECK(st_deep[rec[p].chain0 + c] == p);
}

static void one_case(size_t n, unsigned seed) {
    VerifyBatchGeometry G;
    G.query_words = 37 + seed % 5;   // odd and even: the sections are padded to even words
    G.n_oracles = 4 + seed % 4;
    G.cap_words = 8;
    G.term_words = 3 * (11 + seed % 3);
    G.set_words = 6 * 3;
    G.fri_words = 2 * (G.n_oracles - 4) + 2;
    G.final_degree = 1 + seed % 3;
    std::vector<uint32_t> nq(n);
    uint32_t x = 12345u + seed;
    for (size_t i = 0; i < n; i++) {   // ragged: 1..100, with runs that end exactly on a wave boundary
        x = x * 1664525u + 1013904223u;
        nq[i] = seed % 2 ? 1 + (x >> 16) % 100 : (i % 3 == 0 ? 64 : 1 + (x >> 16) % 7);
    }
    VerifyBatchPlan P;
    CHECK(plan_verify_batch(G, nq.data(), n, &P));
    CHECK(P.records.size() == n && P.tables.size() == n);
    std::vector<unsigned char> owner(P.total_words, 0);
    std::vector<size_t> expect;
    uint64_t chains = 0;
    for (size_t i = 0; i < n; i++) {
        const VerifyBatchProof &R = P.records[i];
        const VerifyTables t = verify_tables(G, nq[i]);
        CHECK(R.chain0 == chains && R.nq == nq[i]);
        claim(owner, R.queries, (size_t)nq[i] * G.query_words, 1);
        claim(owner, P.tables[i], t.words, 2);
        CHECK(P.tables[i] >= P.host_block && P.tables[i] + t.words <= P.host_block + P.host_words);
        CHECK(R.indices == P.tables[i] + t.idx && R.indices + 2 * nq[i] <= R.caps && R.caps + G.n_oracles * G.cap_words <= R.terms);
        CHECK(R.terms + G.term_words <= R.sets && R.sets + G.set_words <= R.fri_ch && R.fri_ch + G.fri_words <= R.final0);
        CHECK(R.final0 + G.final_degree == R.final1 && R.final1 + G.final_degree <= P.tables[i] + t.words);
        for (uint32_t c = 0; c < nq[i]; c++) expect.push_back(i);
        chains += nq[i];
    }
    CHECK(P.n_chains == chains);
    claim(owner, P.record_table, n * VERIFY_BATCH_RECORD_WORDS, 3);
    CHECK(P.record_table + n * VERIFY_BATCH_RECORD_WORDS == P.host_block + P.host_words);
    claim(owner, P.status_open, (G.n_oracles * chains + 1) / 2, 4);
    claim(owner, P.status_deep, (chains + 1) / 2, 5);
    claim(owner, P.record_table2, n * VERIFY_BATCH_RECORD_WORDS, 6);

    // the device block: exactly total_words on the heap, every access below is the sanitizer's to judge
    uint64_t *D = (uint64_t *)std::malloc(P.total_words * 8);
    CHECK(D);
    std::memset(D, 0, P.total_words * 8);
    std::vector<uint64_t> section(100 * G.query_words, 7);
    for (size_t i = 0; i < n; i++) std::memcpy(D + P.records[i].queries, section.data(), (size_t)nq[i] * G.query_words * 8);
    std::vector<uint64_t> block(P.host_words, 9);
    std::memcpy(block.data() + (P.record_table - P.host_block), P.records.data(), n * sizeof(VerifyBatchProof));
    std::memcpy(D + P.host_block, block.data(), block.size() * 8);
    const VerifyBatchProof *d_rec = (const VerifyBatchProof *)(D + P.record_table);
    std::vector<VerifyBatchProof> rec(d_rec, d_rec + n);
    run_pass(G, rec, P.n_chains, D, P.total_words, P.status_open, P.status_deep, expect);

    // second pass over a ragged subset (every third proof, and the last one)
    std::vector<size_t> subset;
    for (size_t i = 0; i < n; i += 3) subset.push_back(i);
    if (subset.back() != n - 1) subset.push_back(n - 1);
    std::vector<VerifyBatchProof> second;
    const uint32_t chains2 = plan_verify_second_pass(P, subset, &second);
    CHECK(second.size() == subset.size() && chains2 <= P.n_chains);
    std::vector<size_t> expect2;
    for (size_t j = 0; j < subset.size(); j++) {
        CHECK(second[j].indices == P.records[subset[j]].indices + nq[subset[j]] && second[j].queries == P.records[subset[j]].queries);
        for (uint32_t c = 0; c < second[j].nq; c++) expect2.push_back(j);
    }
    std::memcpy(D + P.record_table2, second.data(), second.size() * sizeof(VerifyBatchProof));
    run_pass(G, second, chains2, D, P.total_words, P.status_open, P.status_deep, expect2);
    std::free(D);
}

int main() {
    const size_t sizes[] = {1, 2, 63, 64, 65, 1000};
    unsigned cases = 0;
    for (size_t n : sizes)
        for (unsigned seed = 0; seed < 4; seed++, cases++) one_case(n, seed);
    // the limits: one proof too many, one chain too many
    VerifyBatchGeometry G;
    G.query_words = 1;
    VerifyBatchPlan P;
    std::vector<uint32_t> many(VERIFY_BATCH_MAX_PROOFS + 1, 1);
    CHECK(!plan_verify_batch(G, many.data(), many.size(), &P));
    const uint32_t huge[2] = {0x7FFFFFFFu, 1};
    CHECK(!plan_verify_batch(G, huge, 2, &P) && P.records.empty());
    std::printf("ok %u\n", cases);
    return 0;
}
