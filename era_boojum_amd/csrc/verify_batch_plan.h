// bj_verify_batch (and bj_verify, its batch of one): where everything of a batch lies in the context's scratch, and the per-proof
// records the two verifier kernels read (verify_open.h, verifier.hip).  Plain C++ without a device type in it: a stand-alone host program builds it under the
// address and undefined-behaviour sanitizers (tests/verify_batch_plan_check.cpp).
//
// Scratch, in words from its base:   query sections of the proofs, back to back | the proofs' table blocks | record table of the
// first pass | status words of the openings [n_oracles][n_chains] | status words of DEEP / FRI [n_chains] | record table of the
// second pass.  Everything from the first table block to the end of the first record table is built on the host as ONE block
// and crosses in one copy.  All proofs of a batch share the key, so every size but the query count is the batch's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bj {

// One proof of a batch as the two kernels find it: every offset is in words from the base of the batch's scratch.
// chain0 is the prefix sum of nq over the records before this one: the proof's first chain of the launch and its first status slot.
struct VerifyBatchProof {
    uint32_t chain0, nq;
    uint64_t queries;     // [nq][query_words]
    uint64_t indices;     // [nq]: the indices this launch judges the proof at
    uint64_t caps;        // the proof's caps, VerifyOracle::cap_off inside
    uint64_t terms, sets, fri_ch, final0, final1;   // the DEEP / FRI tables
};
static_assert(sizeof(VerifyBatchProof) == 72 && sizeof(VerifyBatchProof) % 8 == 0, "records are copied as words");
constexpr size_t VERIFY_BATCH_RECORD_WORDS = sizeof(VerifyBatchProof) / 8;
constexpr size_t VERIFY_BATCH_MAX_PROOFS = (size_t)1 << 16;

struct VerifyBatchGeometry {   // what the key fixes
    size_t query_words = 0, n_oracles = 0, cap_words = 0, term_words = 0, set_words = 0, fri_words = 0, final_degree = 0;
};
// a proof's table block: drawn indices, stored indices | caps of every oracle | terms | sets | FRI challenges | final monomials,
// each at an even word
struct VerifyTables {
    size_t idx = 0, caps = 0, terms = 0, sets = 0, fri_ch = 0, fm = 0, words = 0;
};
inline size_t verify_padded(size_t words) { return (words + 1) & ~(size_t)1; }
inline VerifyTables verify_tables(const VerifyBatchGeometry &G, size_t nq) {
    VerifyTables t;
    size_t off = 0;
    auto take = [&off](size_t words) {
        const size_t at = off;
        off += verify_padded(words);
        return at;
    };
    t.idx = take(2 * nq);
    t.caps = take(G.n_oracles * G.cap_words);
    t.terms = take(G.term_words);
    t.sets = take(G.set_words);
    t.fri_ch = take(G.fri_words);
    t.fm = take(2 * G.final_degree);
    t.words = off;
    return t;
}

struct VerifyBatchPlan {
    std::vector<VerifyBatchProof> records;   // first pass: the drawn indices
    std::vector<size_t> tables;              // word offset of each proof's table block
    size_t host_block = 0, host_words = 0;   // [host_block, host_block + host_words): table blocks and record table
    size_t record_table = 0, status_open = 0, status_deep = 0, record_table2 = 0, total_words = 0;
    uint32_t n_chains = 0;
};

// nq[i] query openings for proof i of the n that reached the device.  false: the chains do not fit the 32-bit chain index (or n
// is above the limit of a call); nothing is planned then.
inline bool plan_verify_batch(const VerifyBatchGeometry &G, const uint32_t *nq, size_t n, VerifyBatchPlan *P) {
    *P = VerifyBatchPlan{};
    if (n > VERIFY_BATCH_MAX_PROOFS) return false;
    uint64_t chains = 0;
    for (size_t i = 0; i < n; i++) chains += nq[i];
    if (chains >= ((uint64_t)1 << 31)) return false;
    P->records.resize(n);
    P->tables.resize(n);
    size_t off = 0;
    uint32_t chain = 0;
    for (size_t i = 0; i < n; i++) {
        P->records[i].chain0 = chain;
        P->records[i].nq = nq[i];
        P->records[i].queries = off;
        off += verify_padded((size_t)nq[i] * G.query_words);
        chain += nq[i];
    }
    P->n_chains = chain;
    P->host_block = off;
    for (size_t i = 0; i < n; i++) {
        const VerifyTables t = verify_tables(G, nq[i]);
        VerifyBatchProof &r = P->records[i];
        P->tables[i] = off;
        r.indices = off + t.idx;
        r.caps = off + t.caps;
        r.terms = off + t.terms;
        r.sets = off + t.sets;
        r.fri_ch = off + t.fri_ch;
        r.final0 = off + t.fm;
        r.final1 = off + t.fm + G.final_degree;
        off += t.words;
    }
    P->record_table = off;
    off += n * VERIFY_BATCH_RECORD_WORDS;
    P->host_words = off - P->host_block;
    P->status_open = off;
    off += verify_padded((G.n_oracles * (size_t)chain + 1) / 2);
    P->status_deep = off;
    off += verify_padded(((size_t)chain + 1) / 2);
    P->record_table2 = off;
    off += n * VERIFY_BATCH_RECORD_WORDS;
    P->total_words = off;
    return true;
}

// the records of a second pass over `subset` (ascending positions in the first plan): the same blocks judged at the stored
// indices, chains renumbered from 0.  Returns the chains of that launch.
inline uint32_t plan_verify_second_pass(const VerifyBatchPlan &P, const std::vector<size_t> &subset, std::vector<VerifyBatchProof> *out) {
    out->clear();
    uint32_t chain = 0;
    for (size_t i : subset) {
        VerifyBatchProof r = P.records[i];
        r.chain0 = chain;
        r.indices += r.nq;   // the stored indices follow the drawn ones
        chain += r.nq;
        out->push_back(r);
    }
    return chain;
}

// host model of verify_batch_proof_of (verify_open.h): the record chain g belongs to
inline size_t verify_batch_proof_of_host(const VerifyBatchProof *records, size_t n, uint32_t g) {
    size_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) >> 1;
        if (records[mid].chain0 <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace bj
