// bj_vk_* / bj_verify: Verifier::verify (src/cs/implementations/verifier.rs:888-2524) for the circuit class bj_prove handles.
//
// Host (tiny data, order-critical, on top of host_transcript.hpp): the transcript replay (:924-1076), the split of the openings
// (:1150-1206), the challenge powers in the order lookup | specialized | general | L1 | chunks (:1000-1060), the lookup sum
// (:1236-1256), the quotient identity at z (:1090-1810) — hand-written kinds by formula, op lists interpreted over F_p^2 in the
// canonical form of gate_canon.h, the two flattened Poseidon gates by the walks of poseidon_gate_terms.h over F_p^2 — the DEEP
// and FRI challenges (:1819-1955), the proof of work (:1957-1983), the public-input tuples and the query indices.
// Device (the verifier's only volume, ~200 dependent permutations per query): verify_openings (verify_open.h, one kernel per tree
// hasher) walks every Merkle chain; verify_deep_fri_kernel here, one wave per (proof, query), simulates the DEEP value from the four
// opened leaves (:2233-2290), folds it through the schedule (:2387-2519) and compares with the final monomials at the point.
// Both write one status word per chain / query; the host reduces them to the report (include/boojum_hip.h has the order).
//
// The host half is prepare() — named stages from the proof's shape to the tables the kernels read, no context in it, so
// bj_verify_batch runs it for N proofs on worker threads.  The device half is judge(): every proof that got as far, in one launch of
// each kernel (verify_batch_plan.h lays them out in the context's scratch).  bj_verify is that path with one proof.
#include "ctx.h"
#include "gate_program.h"
#include "host_transcript.hpp"
#include "setup.h"
#include "verify_open.h"

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using gl::e2;
using gl::u64;
using VerifyTiming = bj_ctx::VerifyTiming;

namespace bj {
void launch_verify_openings(int hasher, const VerifyOpenArgs &args, hipStream_t s);   // tree_hash.hip
const std::vector<u64> &proof_words(const bj_proof *p);   // prover.hip: the serialised words a proof handle holds
}

struct bj_vk : bj::CircuitShape {   // proof_layout.h
    bj::ProofLayout layout;         // of this shape
    struct Program {   // canonical op list, packed as the interpreter kernels take it (gate_program.h: pack_program)
        std::vector<bj::DevRelation> rel;
        std::vector<u64> values;
        unsigned n_slots = 0;
    };
    struct Gate : bj::GateShape {   // gate_list.h
        Program prog;
    };
    std::vector<Gate> gates, spec;
    unsigned n_gate_terms = 0, n_spec_terms = 0;
    std::vector<u64> non_residues;
    std::vector<unsigned> pub_cols, pub_rows;
    unsigned fri_lde = 0, security = 0, pow_bits = 0, transcript = BJ_TRANSCRIPT_POSEIDON2, hasher = BJ_HASHER_POSEIDON2,
             pow_runner = BJ_POW_BLAKE2S256;
    std::vector<u64> cap;
};

namespace {

const e2 ZERO2{0, 0}, ONE2{1, 0};
e2 e2c(const u64 *p) { return {gl::canon(p[0]), gl::canon(p[1])}; }
e2 base2(u64 x) { return {gl::canon(x), 0}; }
bool eq2(e2 a, e2 b) { return a.c0 == b.c0 && a.c1 == b.c1; }

unsigned slots_of(const std::vector<bj::DevRelation> &rel) {
    unsigned n = 0;
    for (const auto &r : rel)
        if (r.op != bj::canon::OP_WRITE && r.dst + 1 > n) n = r.dst + 1;
    return n;
}

// one repetition of an op list over F_p^2 (Relation / Index of gpu_synthesizer/mod.rs:113-133); false for an operand outside the
// opened columns (the key was checked against its geometry, so this is a defence, not a path)
bool program_terms(const bj_vk::Program &P, const e2 *var, size_t n_var, const e2 *con, size_t n_con, const e2 *wit, size_t n_wit,
                   std::vector<e2> &slots, e2 *terms, unsigned n_terms) {
    slots.assign(P.n_slots ? P.n_slots : 1, ZERO2);
    bool ok = true;
    auto get = [&](uint32_t x) -> e2 {
        const uint32_t k = x >> 28, i = x & 0x0FFFFFFFu;
        switch (k) {
            case BJ_IDX_VARIABLE_POLY: if (i < n_var) return var[i]; break;
            case BJ_IDX_WITNESS_POLY: if (i < n_wit) return wit[i]; break;
            case BJ_IDX_CONSTANT_POLY: if (i < n_con) return con[i]; break;
            case BJ_IDX_TEMPORARY: if (i < slots.size()) return slots[i]; break;
            case BJ_IDX_CONSTANT_VALUE: if (i < P.values.size()) return base2(P.values[i]); break;
            default: break;
        }
        ok = false;
        return ZERO2;
    };
    for (const auto &r : P.rel) {
        const e2 a = get(r.a);
        if (r.op == bj::canon::OP_WRITE) {
            if (r.dst < n_terms) terms[r.dst] = a;
            else ok = false;
            continue;
        }
        e2 v = ZERO2;
        switch (r.op) {
            case BJ_OP_ADD: v = gl::e2_add(a, get(r.b)); break;
            case BJ_OP_DOUBLE: v = gl::e2_add(a, a); break;
            case BJ_OP_SUB: v = gl::e2_sub(a, get(r.b)); break;
            case BJ_OP_NEGATE: v = gl::e2_sub(ZERO2, a); break;
            case BJ_OP_MUL: v = gl::e2_mul(a, get(r.b)); break;
            case BJ_OP_SQUARE: v = gl::e2_sqr(a); break;
            case BJ_OP_INVERSE: v = gl::e2_inv(a); break;   // inverse of 0 is 0, as in the kernels
            default: ok = false; break;
        }
        if (r.dst < slots.size()) slots[r.dst] = v;
        else ok = false;
    }
    return ok;
}

// ---------------------------------------------------------------------------------------------------------------------------
// device: DEEP value, fold chain, final monomials — one wave per query
// ---------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t NO_C1 = 0xFFFFFFFFu;        // a term whose source is a base-field column
constexpr uint32_t DEEP_FINAL = 0x10000u;      // status: 0 ok, 1 + l = the value carried into layer l is not in its leaf, DEEP_FINAL

struct VerifyDeepShared {   // what the key fixes: the same for every proof of a batch
    const u64 *roots;     // inverse bit-reversed twiddles of the 2^log_full domain
    uint32_t query_words, n_sets, n_fri, final_degree, log_full, total_folds;
    u64 omega, kappa;     // generator of the 2^log_full domain; 1 / 7
    uint32_t fri_off[32];
    unsigned char sched[32];
};
// the per-proof tables come out of the record table (verify_batch_plan.h), as word offsets from `base`: queries and indices as in
// verify_open.h; terms [n_terms][3]: leaf word of c0 | leaf word of c1 << 32 (NO_C1: base field), challenge power (c0, c1); sets
// [n_sets][6]: first term, end term, the point (c0, c1), sum_k ch_k * value_k (c0, c1); fri_ch [n_fri][2]; the final monomials
struct VerifyDeepArgs {
    const u64 *base;
    const bj::VerifyBatchProof *proofs;   // [n_proofs], chain0 ascending
    uint32_t *status;     // [n_chains]
    uint32_t n_proofs, n_chains;
    VerifyDeepShared sh;
};

__device__ __forceinline__ u64 shfl64(u64 v, unsigned src) { return (u64)__shfl((unsigned long long)v, (int)src); }
__device__ __forceinline__ e2 shfl2(e2 v, unsigned src) { return {shfl64(v.c0, src), shfl64(v.c1, src)}; }
__device__ __forceinline__ e2 wave_sum(e2 v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        const e2 o{(u64)__shfl_xor((unsigned long long)v.c0, m), (u64)__shfl_xor((unsigned long long)v.c1, m)};
        v = gl::e2_add(v, o);
    }
    return v;
}

// the status word of one query (DEEP_FINAL above); the whole wave calls it and every lane returns the same word
__device__ __forceinline__ uint32_t deep_fri_status(const VerifyDeepShared &A, const u64 *Q, u64 idx, const u64 *terms, const u64 *sets,
                                                    const u64 *fri_ch, const u64 *final0, const u64 *final1, unsigned lane) {
    const u64 x = gl::mul(gl::GEN, gl::pow(A.omega, (u64)gl::bitrev32((gl::u32)idx, A.log_full)));   // x_I = g * w^bitrev(I)
    // h = sum over the opening sets of [ sum_k ch_k f_k(x) - sum_k ch_k v_k ] / (x - at): source order of verifier.rs:2233-2290, one
    // inversion per set; the sources of a set are spread over the lanes
    e2 h{0, 0};
    for (unsigned s = 0; s < A.n_sets; s++) {
        const u64 *S = sets + 6 * (size_t)s;
        e2 acc{0, 0};
        for (u64 t = S[0] + lane; t < S[1]; t += 64) {
            const u64 *T = terms + 3 * t;
            const uint32_t o0 = (uint32_t)T[0], o1 = (uint32_t)(T[0] >> 32);
            const e2 ch{T[1], T[2]};
            const u64 a = gl::canon(Q[o0]);
            acc = gl::e2_add(acc, o1 == NO_C1 ? gl::e2_mul_base(ch, a) : gl::e2_mul(ch, e2{a, gl::canon(Q[o1])}));
        }
        acc = wave_sum(acc);
        const e2 den{gl::sub(x, S[2]), gl::neg(S[3])};
        h = gl::e2_add(h, gl::e2_mul(gl::e2_sub(acc, e2{S[4], S[5]}), gl::e2_inv(den)));
    }
    // the fold chain (verifier.rs:2387-2519), the prover's convention (fri.hip): element i of a leaf lives in lane i; one fold takes
    // lanes (2i, 2i + 1) to lane i with roots[leaf * outs + i] * kappa, kappa squared per fold, the challenge squared inside a step
    uint32_t status = 0;
    e2 cur = h;
    u64 fidx = idx, kappa = A.kappa;
    for (unsigned l = 0; l < A.n_fri; l++) {
        const unsigned k = A.sched[l], m = 1u << k;
        const unsigned sub = (unsigned)fidx & (m - 1);
        const u64 tree = fidx >> k;
        const u64 *L = Q + A.fri_off[l];
        e2 v{0, 0};
        if (lane < m) v = e2{gl::canon(L[lane]), gl::canon(L[m + lane])};
        const e2 carried = shfl2(v, sub);
        if (!status && (carried.c0 != cur.c0 || carried.c1 != cur.c1)) status = 1 + l;
        e2 chal{fri_ch[2 * l], fri_ch[2 * l + 1]};
        for (unsigned f = 0; f < k; f++) {
            const unsigned outs = m >> (f + 1);
            const e2 a = shfl2(v, (2 * lane) & 63), b = shfl2(v, (2 * lane + 1) & 63);
            u64 r = lane < outs ? gl::canon(A.roots[tree * outs + lane]) : 0;
            r = gl::mul(r, kappa);
            const e2 t = gl::e2_mul(gl::e2_mul_base(gl::e2_sub(a, b), r), chal);
            v = e2{gl::add(gl::add(t.c0, a.c0), b.c0), gl::add(gl::add(t.c1, a.c1), b.c1)};
            chal = gl::e2_sqr(chal);
            kappa = gl::sqr(kappa);
        }
        cur = shfl2(v, 0);
        fidx = tree;
    }
    u64 xx = x;
    for (unsigned i = 0; i < A.total_folds; i++) xx = gl::sqr(xx);
    e2 acc{0, 0};
    for (unsigned j = A.final_degree; j-- > 0;) acc = gl::e2_add(gl::e2_mul_base(acc, xx), e2{final0[j], final1[j]});
    if (!status && (acc.c0 != cur.c0 || acc.c1 != cur.c1)) status = DEEP_FINAL;
    return status;
}

// one wave per (proof, query) of the whole launch; the search is over a wave-uniform chain, so it is scalar
__global__ void __launch_bounds__(64) verify_deep_fri_kernel(VerifyDeepArgs A) {
    const unsigned g = blockIdx.x, lane = threadIdx.x;
    if (g >= A.n_chains) return;
    const bj::VerifyBatchProof P = A.proofs[bj::verify_batch_proof_of(A.proofs, A.n_proofs, g)];
    const unsigned c = g - P.chain0;
    if (c >= P.nq) return;
    const u64 *B = A.base;
    const uint32_t status = deep_fri_status(A.sh, B + P.queries + (size_t)c * A.sh.query_words, B[P.indices + c], B + P.terms, B + P.sets,
                                            B + P.fri_ch, B + P.final0, B + P.final1, lane);
    if (lane == 0) A.status[g] = status;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
struct Failure {
    uint32_t stage = BJ_VERIFY_OK, query = 0, oracle = 0;
};

int verdict(bj_verify_report *out, uint32_t stage, uint32_t query = 0, uint32_t oracle = 0, uint32_t checked = 0) {
    out->stage = stage;
    out->query = query;
    out->oracle = oracle;
    out->queries_checked = checked;
    return BJ_OK;
}

bool pow_holds(unsigned runner, const u64 *seed5, unsigned bits, u64 nonce) {   // POW::verify_from_field_elements (pow.rs:16-31)
    unsigned char msg[48], out[32];
    for (int i = 0; i < 5; i++)
        for (int b = 0; b < 8; b++) msg[8 * i + b] = (unsigned char)(seed5[i] >> (8 * b));
    for (int b = 0; b < 8; b++) msg[40 + b] = (unsigned char)(nonce >> (8 * b));
    if (runner == BJ_POW_KECCAK256) {
        bj::host::Keccak256 h;
        h.update(msg, 48);
        h.finalize_reset(out);
    } else {
        bj::host::Blake2s h;
        h.update(msg, 48);
        h.finalize_reset(out);
    }
    u64 first = 0;
    for (int b = 0; b < 8; b++) first |= (u64)out[b] << (8 * b);
    const unsigned tz = first ? (unsigned)__builtin_ctzll(first) : 64u;
    return tz >= bits;
}

// What the key fixes about the device work, as prepare() works it out: the same in every proof of a batch.
struct Geometry {
    bj::VerifyBatchGeometry sizes;
    unsigned LOGN = 0, n_sets = 0, n_fri = 0, total_folds = 0;
    bj::VerifyOracle oracle[bj::VERIFY_MAX_ORACLES] = {};
    uint32_t fri_off[32] = {};
    unsigned char sched[32] = {};
};
// A proof after the host half.  device == false: `report` is the verdict (or rc < 0 and err say why there is none).  device ==
// true: the host checks passed; the tables (verify_batch_plan.h: verify_tables) and the query section wait for the judge.
struct Prepared {
    int rc = BJ_OK;
    std::string err;
    bj_verify_report report = {};
    bool device = false;
    size_t nq = 0;
    int first_mismatch = -1;       // first query whose stored index is not the drawn one
    const u64 *queries = nullptr;  // the query section, inside the caller's buffer
    std::vector<u64> tables;
    Geometry geo;
    int refuse(int code, const char *fmt, ...) {
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return rc = code;
    }
};

// ---- the stages of prepare(), in the order it runs them.  A stage that returns bool has put the verdict (or the refusal) into
// the Prepared when it returns false; what one stage hands to the next is in the plain structs below ----

// The counts the key dictates and where the sections of one proof lie (pointers into the caller's buffer).
struct ProofView {
    bj::SerialLayout at;   // proof_layout.h: the sections, the words of a query
    unsigned log_n, V, Wc, nC, q, log_fri, LOGN, n_chunks, n_lookup_terms;
    bool has_lookup;
    size_t N, cap, nz, n_pub, nq, sched_len, final_degree;
    uint32_t sched[32], new_pow;
    u64 pow_challenge;
    const u64 *pub, *wit_cap, *s2_cap, *q_cap, *vz_w, *vzo_w, *v0_w, *fri_caps, *fm0, *fm1, *queries;
};
struct Challenges { e2 beta, gamma, lbeta, lgamma, alpha, z; };
// The values the proof claims at z, z * omega and 0, split by kind (verifier.rs:1150-1206); the pointers go into vz.
struct Openings {
    std::vector<e2> vz, v0;
    e2 z_at_zo, z_at_z;
    const e2 *var_z, *wit_z, *con_z, *sig_z, *part_z, *mult_z, *A_z, *B_z, *tab_z, *qch_z;
};
// What the transcript yields after the quotient identity: the DEEP and FRI challenges and the query indices.
struct Draw {
    e2 cch = ZERO2;
    std::vector<u64> fri_ch;    // [sched_len][2]
    std::vector<u64> indices;   // [nq] drawn, then [nq] stored: the proof's claim
    int first_mismatch = -1;
};
// The DEEP sources in opening order as the kernel reads them (VerifyDeepArgs: terms, sets).
struct DeepTables {
    std::vector<u64> term_words, set_words;
    size_t n_sets = 0;
};

e2 challenge2(bj::host::Transcript &t) {
    const u64 a = t.challenge(), b = t.challenge();
    return e2{gl::canon(a), gl::canon(b)};
}

// shape: every count is the key's before it sizes anything
bool parse_proof(const bj_vk *K, const u64 *W, size_t n_words, unsigned flags, Prepared *R, ProofView *P) {
    bj_verify_report *out = &R->report;
    const bj::ProofLayout &L = K->layout;
    P->V = K->V, P->Wc = K->Wc, P->nC = K->nC, P->q = K->q;
    const unsigned log_n = P->log_n = K->log_n, log_fri = P->log_fri = K->log_fri;
    P->LOGN = log_n + log_fri;
    P->N = (size_t)1 << P->LOGN, P->cap = K->cap_size;
    P->has_lookup = L.has_lookup;
    P->n_chunks = L.n_chunks, P->n_lookup_terms = L.n_lookup_terms, P->nz = L.nz;
    uint32_t *sched = P->sched;
    size_t num_queries = 0, sched_len = 0, final_degree = 0;
    if (bj_fri_schedule(K->security, P->cap, K->pow_bits, log_fri, log_n, &P->new_pow, &num_queries, sched, &sched_len, &final_degree) || sched_len > 32) {
        R->refuse(BJ_ERR_INVALID_ARG, "bj_verify: compute_fri_schedule failed for the key's config");
        return false;
    }
    P->sched_len = sched_len;
    P->final_degree = final_degree;
    auto shape = [&]() { verdict(out, BJ_VERIFY_SHAPE); return false; };
    const size_t n_pub = P->n_pub = K->pub_cols.size();
    if (!W || n_words < bj::ProofHeader::WORDS) return shape();
    const u64 nq64 = W[bj::ProofHeader::N_QUERIES];
    const bool partial = (flags & BJ_VERIFY_PARTIAL_QUERIES) != 0;
    if (!(nq64 == num_queries || (partial && nq64 > 0 && nq64 < num_queries))) return shape();
    const size_t nq = P->nq = (size_t)nq64;
    const bj::SerialLayout &at = P->at = bj::serial_layout(L, sched, sched_len, final_degree, nq, n_pub);
    if (!at.ok) return shape();   // a domain below the cap, a schedule the prover cannot emit
    bj::ProofHeader header;
    header.fill(L, n_pub, sched_len, final_degree, nq, at.depth, K->pow_bits, 0);
    if (!header.matches(W) || n_words != at.total) return shape();
    P->pow_challenge = W[bj::ProofHeader::POW_CHALLENGE];
    for (size_t l = 0; l < sched_len; l++)
        if (W[at.schedule + l] != sched[l]) return shape();
    P->pub = W + at.public_inputs;
    P->wit_cap = W + at.witness_cap;
    P->s2_cap = W + at.stage2_cap;
    P->q_cap = W + at.quotient_cap;
    P->vz_w = W + at.values_at_z;
    P->vzo_w = W + at.values_at_z_omega;
    P->v0_w = W + at.values_at_0;
    P->fri_caps = W + at.fri_caps;
    P->fm0 = W + at.final_c0;
    P->fm1 = W + at.final_c1;
    P->queries = W + at.queries;
    return true;
}

// transcript replay up to the openings (verifier.rs:924-1076); `t` goes on to draw_challenges_and_indices
Challenges replay_transcript(const bj_vk *K, const ProofView &P, bj::host::Transcript &t) {
    Challenges C{};
    t.kind = (int)K->transcript;
    t.absorb_cap(K->cap.data(), K->cap.size());
    t.absorb(P.pub, P.n_pub);
    t.absorb_cap(P.wit_cap, P.cap * 4);
    C.beta = challenge2(t);
    C.gamma = challenge2(t);
    if (P.has_lookup) {
        C.lbeta = challenge2(t);
        C.lgamma = challenge2(t);
    }
    t.absorb_cap(P.s2_cap, P.cap * 4);
    C.alpha = challenge2(t);
    t.absorb_cap(P.q_cap, P.cap * 4);
    C.z = challenge2(t);
    t.absorb(P.vz_w, 2 * P.nz);
    t.absorb(P.vzo_w, 2);
    t.absorb(P.v0_w, 2 * (size_t)P.n_lookup_terms);
    return C;
}

// the openings, split (verifier.rs:1150-1206)
void split_openings(const bj_vk *K, const ProofView &P, Openings *O) {
    O->vz.resize(P.nz);
    O->v0.resize(P.n_lookup_terms);
    for (size_t i = 0; i < P.nz; i++) O->vz[i] = e2c(P.vz_w + 2 * i);
    for (size_t i = 0; i < P.n_lookup_terms; i++) O->v0[i] = e2c(P.v0_w + 2 * i);
    O->z_at_zo = e2c(P.vzo_w);
    const bj::ProofLayout &L = K->layout;
    const e2 *vz = O->vz.data();
    O->var_z = vz + L.at_var;
    O->wit_z = vz + L.at_wit;
    O->con_z = vz + L.at_const;
    O->sig_z = vz + L.at_sigma;
    O->z_at_z = vz[L.at_z];
    O->part_z = vz + L.at_partial;
    O->mult_z = vz + L.at_mult;
    O->A_z = vz + L.at_a;
    O->B_z = vz + L.at_b;
    O->tab_z = vz + L.at_table;
    O->qch_z = vz + L.at_chunk;
}

// the lookup sub-arguments at z (verifier.rs:1397-1470)
e2 lookup_terms(const bj_vk *K, const Challenges &C, const Openings &O, const e2 *a_lookup) {
    e2 T = ZERO2;
    std::vector<e2> gp(K->lookup_w + 1);
    gp[0] = ONE2;
    for (unsigned j = 1; j <= K->lookup_w; j++) gp[j] = gl::e2_mul(gp[j - 1], C.lgamma);
    for (unsigned i = 0; i < K->lookup_reps; i++) {
        e2 d = C.lbeta;
        for (unsigned j = 0; j < K->lookup_cps; j++) d = gl::e2_add(d, gl::e2_mul(gp[j], O.var_z[K->layout.lookup_var(i, j)]));
        if (!K->tid_var) d = gl::e2_add(d, gl::e2_mul(gp[K->lookup_w], O.con_z[K->table_id_col]));
        T = gl::e2_add(T, gl::e2_mul(gl::e2_sub(gl::e2_mul(O.A_z[i], d), ONE2), a_lookup[i]));
    }
    e2 d = C.lbeta;
    for (unsigned j = 0; j <= K->lookup_w; j++) d = gl::e2_add(d, gl::e2_mul(gp[j], O.tab_z[j]));
    return gl::e2_add(T, gl::e2_mul(gl::e2_sub(gl::e2_mul(O.B_z[0], d), O.mult_z[0]), a_lookup[K->lookup_reps]));
}

// gates over specialized columns: no selector, their own columns (verifier.rs:1560-1638)
e2 specialized_gate_terms(const bj_vk *K, const Openings &O, const e2 *a_spec, bool *well_formed) {
    e2 T = ZERO2;
    std::vector<e2> slots, terms;
    for (const auto &g : K->spec) {
        terms.assign(g.num_terms ? g.num_terms : 1, ZERO2);
        for (unsigned r = 0; r < g.reps; r++) {
            const size_t vb = g.first_col + (size_t)r * g.var_stride, cb = g.first_const + (size_t)r * g.const_stride;
            *well_formed = program_terms(g.prog, O.var_z + vb, g.var_stride, O.con_z + cb, g.const_stride, nullptr, 0, slots, terms.data(), g.num_terms) && *well_formed;
            const e2 *a = a_spec + g.first_term + (size_t)r * g.num_terms;
            for (unsigned k = 0; k < g.num_terms; k++) T = gl::e2_add(T, gl::e2_mul(terms[k], a[k]));
        }
    }
    return T;
}

// gates over general-purpose columns under their selectors (verifier.rs:1640-1720)
e2 general_gate_terms(const bj_vk *K, const ProofView &P, const Openings &O, const e2 *a_gates, bool *well_formed) {
    const unsigned nC = P.nC, Wc = P.Wc;
    const e2 *var_z = O.var_z, *wit_z = O.wit_z, *con_z = O.con_z;
    e2 T = ZERO2;
    std::vector<e2> slots, terms;
    for (const auto &g : K->gates) {
        if (!g.num_terms) continue;
        e2 sel = ONE2;
        for (unsigned b = 0; b < g.path_len; b++) sel = gl::e2_mul(sel, g.path[b] ? con_z[b] : gl::e2_sub(ONE2, con_z[b]));
        const unsigned d = g.path_len;
        e2 acc = ZERO2;
        terms.assign(g.num_terms, ZERO2);
        for (unsigned r = 0; r < g.reps; r++) {
            const size_t vb = (size_t)r * g.var_stride, cb = d + (size_t)r * g.const_stride;
            const e2 *v = var_z + vb;
            unsigned n_pushed = 0;   // the walks of poseidon_gate_terms.h read variables and hand over their terms in order
            auto var_at = [&](unsigned k) { return v[k]; };
            auto push_term = [&](e2 t) { terms[n_pushed++] = t; };
            switch (g.kind) {
                case BJ_GATE_CONSTANT_ALLOCATOR: terms[0] = gl::e2_sub(v[0], con_z[cb]); break;
                case BJ_GATE_FMA_NO_CONSTANT:
                    terms[0] = gl::e2_sub(gl::e2_add(gl::e2_mul(v[2], con_z[d + 1]), gl::e2_mul(con_z[d], gl::e2_mul(v[0], v[1]))), v[3]);
                    break;
                case BJ_GATE_REDUCTION4: {
                    e2 s = ZERO2;
                    for (int k = 0; k < 4; k++) s = gl::e2_add(s, gl::e2_mul(v[k], con_z[d + k]));
                    terms[0] = gl::e2_sub(s, v[4]);
                    break;
                }
                case BJ_GATE_POSEIDON2_FLATTENED: bj::poseidon2_flattened_terms<bj::GateE2>(var_at, push_term); break;
                case BJ_GATE_POSEIDON_FLATTENED: bj::poseidon1_flattened_terms<bj::GateE2>(var_at, push_term); break;
                default:   // BJ_GATE_PROGRAM
                    if (vb > K->num_gp_vars || cb > nC || (size_t)r * g.wit_stride > Wc) {
                        *well_formed = false;
                        break;
                    }
                    *well_formed = program_terms(g.prog, v, K->num_gp_vars - vb, con_z + cb, nC - cb, wit_z + (size_t)r * g.wit_stride,
                                                 Wc - (size_t)r * g.wit_stride, slots, terms.data(), g.num_terms) && *well_formed;
                    break;
            }
            const e2 *a = a_gates + g.first_term + (size_t)r * g.num_terms;
            for (unsigned k = 0; k < g.num_terms; k++) acc = gl::e2_add(acc, gl::e2_mul(terms[k], a[k]));
        }
        T = gl::e2_add(T, gl::e2_mul(acc, sel));
    }
    return T;
}

// (z(x) - 1) L1 and the copy-permutation chain (verifier.rs:1722-1790); a_rest: the power of L1, then one per chunk
e2 copy_permutation_terms(const bj_vk *K, const ProofView &P, const Challenges &C, const Openings &O, e2 vanishing, const e2 *a_rest) {
    const e2 z = C.z, beta = C.beta, gamma = C.gamma;
    const e2 l1 = gl::e2_mul(vanishing, gl::e2_inv(gl::e2_sub(z, ONE2)));
    e2 T = gl::e2_mul(gl::e2_mul(gl::e2_sub(O.z_at_z, ONE2), l1), a_rest[0]);
    for (unsigned j = 0; j < P.n_chunks; j++) {
        e2 lhs = j + 1 < P.n_chunks ? O.part_z[j] : O.z_at_zo, rhs = j ? O.part_z[j - 1] : O.z_at_z;
        for (unsigned c = j * P.q; c < (j + 1) * P.q && c < P.V; c++) {
            lhs = gl::e2_mul(lhs, gl::e2_add(gl::e2_add(gl::e2_mul(O.sig_z[c], beta), O.var_z[c]), gamma));
            rhs = gl::e2_mul(rhs, gl::e2_add(gl::e2_add(gl::e2_mul(gl::e2_mul_base(z, gl::canon(K->non_residues[c])), beta), O.var_z[c]), gamma));
        }
        T = gl::e2_add(T, gl::e2_mul(gl::e2_sub(lhs, rhs), a_rest[1 + j]));
    }
    return T;
}

// The lookup sum and the quotient identity at z (verifier.rs:1090-1810): BJ_VERIFY_OK, or the stage that fails.  Challenge
// powers in the order lookup | specialized | general | L1 | chunks (prover.rs:599-625, verifier.rs:1000-1060).
uint32_t quotient_identity(const bj_vk *K, const ProofView &P, const Challenges &C, const Openings &O) {
    const size_t n_gate_terms = K->n_gate_terms, n_spec_terms = K->n_spec_terms;
    const size_t total_terms = P.n_lookup_terms + n_spec_terms + n_gate_terms + 1 + P.n_chunks;
    std::vector<e2> alphas(total_terms);
    alphas[0] = ONE2;
    for (size_t i = 1; i < total_terms; i++) alphas[i] = gl::e2_mul(alphas[i - 1], C.alpha);
    const e2 *a_lookup = alphas.data(), *a_spec = a_lookup + P.n_lookup_terms, *a_gates = a_spec + n_spec_terms, *a_rest = a_gates + n_gate_terms;

    e2 T = ZERO2;
    if (P.has_lookup) {
        e2 sa = ZERO2;   // the sum of the A_i(0) is B(0) (verifier.rs:1236-1256)
        for (unsigned i = 0; i < K->lookup_reps; i++) sa = gl::e2_add(sa, O.v0[i]);
        if (!eq2(sa, O.v0[K->lookup_reps])) return BJ_VERIFY_LOOKUP_SUM;
        T = lookup_terms(K, C, O, a_lookup);
    }
    bool well_formed = true;
    T = gl::e2_add(T, specialized_gate_terms(K, O, a_spec, &well_formed));
    T = gl::e2_add(T, general_gate_terms(K, P, O, a_gates, &well_formed));
    e2 z_n = C.z;
    for (unsigned i = 0; i < P.log_n; i++) z_n = gl::e2_sqr(z_n);
    const e2 vanishing = gl::e2_sub(z_n, ONE2);
    T = gl::e2_add(T, copy_permutation_terms(K, P, C, O, vanishing, a_rest));
    e2 t_chunks = ZERO2, pw = ONE2;
    for (unsigned i = 0; i < P.q; i++) {
        t_chunks = gl::e2_add(t_chunks, gl::e2_mul(O.qch_z[i], pw));
        pw = gl::e2_mul(pw, z_n);
    }
    return well_formed && eq2(T, gl::e2_mul(t_chunks, vanishing)) ? BJ_VERIFY_OK : BJ_VERIFY_QUOTIENT;
}

// DEEP / FRI challenges, proof of work (verifier.rs:1819-1983), then the query indices: drawn in order; the stored words are the
// proof's claim
bool draw_challenges_and_indices(const bj_vk *K, const ProofView &P, bj::host::Transcript &t, Prepared *R, Draw *D) {
    auto stop = [&](uint32_t stage, size_t query) { verdict(&R->report, stage, (uint32_t)query, 0, (uint32_t)query); return false; };
    D->cch = challenge2(t);
    D->fri_ch.resize(2 * P.sched_len);
    for (size_t l = 0; l < P.sched_len; l++) {
        t.absorb_cap(P.fri_caps + l * P.cap * 4, P.cap * 4);
        const e2 ch = challenge2(t);
        D->fri_ch[2 * l] = ch.c0;
        D->fri_ch[2 * l + 1] = ch.c1;
    }
    t.absorb(P.fm0, P.final_degree);
    t.absorb(P.fm1, P.final_degree);
    if (P.new_pow) {
        u64 seed[5];
        for (int i = 0; i < 5; i++) seed[i] = gl::canon(t.challenge());
        if (!pow_holds(K->pow_runner, seed, P.new_pow, P.pow_challenge)) return stop(BJ_VERIFY_POW, 0);
        const u64 lh[2] = {P.pow_challenge & 0xFFFFFFFFULL, P.pow_challenge >> 32};
        t.absorb(lh, 2);
    }
    const size_t nq = P.nq;
    D->indices.resize(2 * nq);
    bj::host::BoolsBuffer bools;
    bools.max_needed = P.LOGN;
    for (size_t i = 0; i < nq; i++) {
        D->indices[i] = bools.query_index(t, P.log_n, P.log_fri);
        const u64 stored = P.queries[i * P.at.query_words];
        if (stored >= P.N) return stop(BJ_VERIFY_SHAPE, i);   // not an index of the domain at all
        D->indices[nq + i] = stored;
        if (stored != D->indices[i] && D->first_mismatch < 0) D->first_mismatch = (int)i;
    }
    return true;
}

// the DEEP sources in opening order (verifier.rs:2233-2290) as words of a query's block
bool deep_tables(const bj_vk *K, const ProofView &P, const Challenges &C, const Openings &O, const Draw &D, Prepared *R, DeepTables *DT) {
    const bj::ProofLayout &L = K->layout;
    const unsigned n_lookup_terms = P.n_lookup_terms, log_n = P.log_n;
    const size_t nz = P.nz, n_pub = P.n_pub;
    struct Term { uint32_t o0, o1; };
    auto term_of = [&](const bj::Opened &o) {   // the words of a query's block that hold the polynomial's leaf elements
        const uint32_t leaf = P.at.leaf_off[o.oracle];
        return Term{leaf + o.col0, o.col1 == bj::NO_COLUMN ? NO_C1 : leaf + o.col1};
    };
    if (L.opened.size() != nz) {
        R->refuse(BJ_ERR_HIP, "bj_verify: internal error: %zu DEEP sources for %zu openings", L.opened.size(), nz);
        return false;
    }
    const std::vector<bj::OpeningSet> sets = L.opening_sets(K->pub_cols.data(), K->pub_rows.data(), n_pub);
    const size_t n_sets = DT->n_sets = sets.size();
    const size_t n_terms = nz + 1 + n_lookup_terms + n_pub;
    std::vector<u64> &term_words = DT->term_words, &set_words = DT->set_words;
    term_words.assign(3 * n_terms, 0);
    set_words.assign(6 * n_sets, 0);
    e2 chp = ONE2;
    size_t tno = 0, sno = 0;
    auto open_set = [&](e2 at) {
        u64 *S = set_words.data() + 6 * sno;
        S[0] = tno; S[2] = at.c0; S[3] = at.c1; S[4] = 0; S[5] = 0;
    };
    auto add_term = [&](Term s, e2 value) {
        u64 *Tw = term_words.data() + 3 * tno++;
        Tw[0] = (u64)s.o0 | ((u64)s.o1 << 32);
        Tw[1] = chp.c0; Tw[2] = chp.c1;
        u64 *S = set_words.data() + 6 * sno;
        const e2 c = gl::e2_add(e2{S[4], S[5]}, gl::e2_mul(chp, value));
        S[4] = c.c0; S[5] = c.c1;
        chp = gl::e2_mul(chp, D.cch);
    };
    auto close_set = [&]() { set_words[6 * sno++ + 1] = tno; };
    auto point_of = [&](const bj::OpeningSet &set) {
        switch (set.point) {
            case bj::OPEN_AT_Z: return C.z;
            case bj::OPEN_AT_Z_OMEGA: return gl::e2_mul_base(C.z, gl::omega(log_n));
            case bj::OPEN_AT_ZERO: return ZERO2;
            default: return e2{gl::pow(gl::omega(log_n), set.row), 0};
        }
    };
    auto value_of = [&](const bj::OpeningSet &set, size_t i) {
        switch (set.point) {
            case bj::OPEN_AT_Z: return O.vz[set.value[i]];
            case bj::OPEN_AT_Z_OMEGA: return O.z_at_zo;
            case bj::OPEN_AT_ZERO: return O.v0[set.value[i]];
            default: return e2{gl::canon(P.pub[set.value[i]]), 0};
        }
    };
    for (const bj::OpeningSet &set : sets) {
        open_set(point_of(set));
        for (size_t i = 0; i < set.polys.size(); i++) add_term(term_of(set.polys[i]), value_of(set, i));
        close_set();
    }
    return true;
}

// what the judge needs: the geometry, and the tables in the block layout of verify_tables
void fill_device_tables(const bj_vk *K, const ProofView &P, const Draw &D, const DeepTables &DT, Prepared *R) {
    const size_t sched_len = P.sched_len, final_degree = P.final_degree, nq = P.nq, n_oracles = 4 + sched_len, cap_words = P.cap * 4;
    const bj::SerialLayout &at_q = P.at;
    const unsigned *widths = K->layout.widths;
    Geometry &G = R->geo;
    G.sizes.query_words = at_q.query_words;
    G.sizes.n_oracles = n_oracles;
    G.sizes.cap_words = cap_words;
    G.sizes.term_words = DT.term_words.size();
    G.sizes.set_words = DT.set_words.size();
    G.sizes.fri_words = D.fri_ch.size();
    G.sizes.final_degree = final_degree;
    G.LOGN = P.LOGN;
    G.n_sets = (unsigned)DT.n_sets;
    G.n_fri = (unsigned)sched_len;
    G.total_folds = at_q.total_folds;
    for (int o = 0; o < 4; o++) G.oracle[o] = bj::VerifyOracle{at_q.leaf_off[o], widths[o], at_q.depth, 0, (uint32_t)(o * cap_words)};
    uint32_t shift = 0;
    for (size_t l = 0; l < sched_len; l++) {
        shift += P.sched[l];
        G.oracle[4 + l] = bj::VerifyOracle{at_q.fri_leaf_off[l], 2u << P.sched[l], at_q.fri_depth[l], shift, (uint32_t)((4 + l) * cap_words)};
        G.fri_off[l] = at_q.fri_leaf_off[l];
        G.sched[l] = (unsigned char)P.sched[l];
    }
    const bj::VerifyTables at = bj::verify_tables(G.sizes, nq);
    R->tables.assign(at.words, 0);
    u64 *s = R->tables.data();
    std::memcpy(s + at.idx, D.indices.data(), D.indices.size() * 8);
    std::memcpy(s + at.caps, P.wit_cap, cap_words * 8);
    std::memcpy(s + at.caps + cap_words, P.s2_cap, cap_words * 8);
    std::memcpy(s + at.caps + 2 * cap_words, P.q_cap, cap_words * 8);
    std::memcpy(s + at.caps + 3 * cap_words, K->cap.data(), cap_words * 8);
    std::memcpy(s + at.caps + 4 * cap_words, P.fri_caps, sched_len * cap_words * 8);
    std::memcpy(s + at.terms, DT.term_words.data(), DT.term_words.size() * 8);
    std::memcpy(s + at.sets, DT.set_words.data(), DT.set_words.size() * 8);
    std::memcpy(s + at.fri_ch, D.fri_ch.data(), D.fri_ch.size() * 8);
    for (size_t i = 0; i < final_degree; i++) {
        s[at.fm + i] = gl::canon(P.fm0[i]);
        s[at.fm + final_degree + i] = gl::canon(P.fm1[i]);
    }
    R->nq = nq;
    R->first_mismatch = D.first_mismatch;
    R->queries = P.queries;
    R->device = true;
}

// The host half: the stages above, first verdict wins.  Touches no context and no global state: bj_verify_batch runs it on
// several threads at once.  Returns R->rc.
int prepare(const bj_vk *K, const u64 *W, size_t n_words, unsigned flags, Prepared *R) {
    ProofView P{};
    if (!parse_proof(K, W, n_words, flags, R, &P)) return R->rc;
    bj::host::Transcript t;
    const Challenges C = replay_transcript(K, P, t);
    Openings O{};
    split_openings(K, P, &O);
    if (const uint32_t stage = quotient_identity(K, P, C, O)) return verdict(&R->report, stage);
    Draw D;
    if (!draw_challenges_and_indices(K, P, t, R, &D)) return R->rc;
    DeepTables DT;
    if (!deep_tables(K, P, C, O, D, R, &DT)) return R->rc;
    fill_device_tables(K, P, D, DT, R);
    return BJ_OK;
}

VerifyDeepShared deep_shared(const bj_ctx *ctx, const Geometry &G) {
    VerifyDeepShared sh{};
    sh.roots = ctx->tw_inv.p;
    sh.query_words = (uint32_t)G.sizes.query_words;
    sh.n_sets = G.n_sets;
    sh.n_fri = G.n_fri;
    sh.final_degree = (uint32_t)G.sizes.final_degree;
    sh.log_full = G.LOGN;
    sh.total_folds = G.total_folds;
    sh.omega = gl::omega(G.LOGN);
    sh.kappa = gl::inv(gl::GEN);
    std::memcpy(sh.fri_off, G.fri_off, sizeof sh.fri_off);
    std::memcpy(sh.sched, G.sched, sizeof sh.sched);
    return sh;
}

// the first failure of one proof in the order of include/boojum_hip.h; st_open is [n_oracles][stride] from this proof's first
// chain on, st_deep [nq]
Failure first_failure(const uint32_t *st_open, size_t stride, const uint32_t *st_deep, size_t nq, size_t n_fri) {
    for (size_t i = 0; i < nq; i++) {
        for (uint32_t o = 0; o < 4; o++)
            if (!st_open[o * stride + i]) return Failure{BJ_VERIFY_MERKLE, (uint32_t)i, o};
        for (uint32_t l = 0; l < n_fri; l++) {
            if (st_deep[i] == 1 + l) return Failure{BJ_VERIFY_FRI_VALUE, (uint32_t)i, l};
            if (!st_open[(4 + l) * stride + i]) return Failure{BJ_VERIFY_FRI_MERKLE, (uint32_t)i, l};
        }
        if (st_deep[i]) return Failure{BJ_VERIFY_FINAL, (uint32_t)i, 0};
    }
    return Failure{};
}

// The verdict over a proof that reached its kernels.  at_drawn: its first failure at the drawn indices.  Returns true when the
// verdict needs the first failure at the stored indices, too (second == nullptr), and uses it when given.
// The stored indices are not the drawn ones and the drawn ones fail: what do the openings the proof carries fail at?  This second
// pass exists for two rows of the stage table alone and never turns a rejection into an acceptance: a final monomial and a FRI
// cap are absorbed BEFORE the indices are drawn, so editing either moves every index — at the drawn indices such a proof fails
// at the witness path of query 0, whatever was edited; BJ_VERIFY_FINAL for the monomial and BJ_VERIFY_FRI_VALUE for a FRI leaf
// whose path (and therefore cap entry) was recomputed can only be told at the indices the prover opened.
bool device_verdict(bj_verify_report *out, size_t nq, int first_mismatch, const Failure &at_drawn, const Failure *at_stored) {
    if (at_drawn.stage == BJ_VERIFY_OK) {
        if (first_mismatch < 0) verdict(out, BJ_VERIFY_OK, 0, 0, (uint32_t)nq);
        else verdict(out, BJ_VERIFY_SHAPE, (uint32_t)first_mismatch, 0, (uint32_t)first_mismatch);
        return false;
    }
    if (first_mismatch < 0) {
        verdict(out, at_drawn.stage, at_drawn.query, at_drawn.oracle, at_drawn.query);
        return false;
    }
    if (!at_stored) return true;
    if (at_stored->stage == BJ_VERIFY_OK) verdict(out, BJ_VERIFY_SHAPE, (uint32_t)first_mismatch, 0, (uint32_t)first_mismatch);
    else verdict(out, at_stored->stage, at_stored->query, at_stored->oracle, at_stored->query);
    return false;
}

// The device half of bj_verify (n == 1) and bj_verify_batch: the proofs of R[0..n) that reached it (R[i].device) judged in one
// launch of each kernel over every chain — plan (verify_batch_plan.h), scratch and twiddles before anything is uploaded, every
// query section and ONE host block of table blocks and records up, two launches, the status words down, the verdicts into out[i];
// then the same pair of launches over the proofs whose verdict needs the stored indices (device_verdict).  out[i] of a proof that
// ended on the host is not touched.  T: the caller's timing state; T->state becomes 2 once the kernels have run.
int judge(bj_ctx *ctx, const bj_vk *K, const Prepared *R, size_t n, bj_verify_report *out, VerifyTiming *T) {
    std::vector<size_t> dev;   // the proofs that reached the device phase, ascending
    std::vector<uint32_t> nqs;
    for (size_t i = 0; i < n; i++)
        if (R[i].device) {
            dev.push_back(i);
            nqs.push_back((uint32_t)R[i].nq);
        }
    if (dev.empty()) return BJ_OK;
    const Geometry &G = R[dev[0]].geo;   // the key's: the same in every proof
    const size_t n_oracles = G.sizes.n_oracles;
    bj::VerifyBatchPlan P;
    if (!bj::plan_verify_batch(G.sizes, nqs.data(), dev.size(), &P))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: the batch has more than 2^31 query openings");
    if (int rc = bj::ensure_scratch(ctx, P.total_words)) return rc;   // before anything is uploaded
    if (int rc = bj::ensure_twiddles(ctx, G.LOGN, true)) return rc;
    u64 *D = ctx->d_scratch.p;
    hipStream_t st = ctx->stream;
    for (auto &e : T->ev)
        if (int rc = bj::ensure_event(ctx, e)) return rc;
    std::vector<u64> block(P.host_words);
    for (size_t k = 0; k < dev.size(); k++)
        std::memcpy(block.data() + (P.tables[k] - P.host_block), R[dev[k]].tables.data(), R[dev[k]].tables.size() * 8);
    std::memcpy(block.data() + (P.record_table - P.host_block), P.records.data(), P.records.size() * sizeof(bj::VerifyBatchProof));
    // stream-ordered copies out of the caller's buffers and `block`: all of them outlive the synchronisation below
    BJ_HIP(ctx, hipEventRecord(T->ev[0], st));
    for (size_t k = 0; k < dev.size(); k++)
        BJ_HIP(ctx, hipMemcpyAsync(D + P.records[k].queries, R[dev[k]].queries, (size_t)nqs[k] * G.sizes.query_words * 8, hipMemcpyHostToDevice, st));
    BJ_HIP(ctx, hipMemcpyAsync(D + P.host_block, block.data(), block.size() * 8, hipMemcpyHostToDevice, st));
    BJ_HIP(ctx, hipEventRecord(T->ev[1], st));
    bj::VerifyOpenArgs OA{};
    OA.base = D;
    OA.status = (uint32_t *)(D + P.status_open);
    OA.query_words = (uint32_t)G.sizes.query_words;
    OA.n_oracles = (uint32_t)n_oracles;
    std::memcpy(OA.oracle, G.oracle, sizeof OA.oracle);
    VerifyDeepArgs DA{};
    DA.base = D;
    DA.status = (uint32_t *)(D + P.status_deep);
    DA.sh = deep_shared(ctx, G);
    std::vector<uint32_t> status;
    // both kernels over `n_records` records at d_records, `chains` chains in all; the status words land in `status`: openings, then DEEP
    auto launch = [&](const u64 *d_records, size_t n_records, uint32_t chains, bool timed) -> int {
        OA.proofs = DA.proofs = (const bj::VerifyBatchProof *)d_records;
        OA.n_proofs = DA.n_proofs = (uint32_t)n_records;
        OA.n_chains = DA.n_chains = chains;
        bj::launch_verify_openings((int)K->hasher, OA, st);
        if (timed) BJ_HIP(ctx, hipEventRecord(T->ev[2], st));
        hipLaunchKernelGGL(verify_deep_fri_kernel, dim3(chains), dim3(64), 0, st, DA);
        if (timed) BJ_HIP(ctx, hipEventRecord(T->ev[3], st));
        BJ_CHECK_LAUNCH(ctx);
        status.resize((n_oracles + 1) * (size_t)chains);
        BJ_HIP(ctx, hipMemcpyAsync(status.data(), OA.status, n_oracles * (size_t)chains * 4, hipMemcpyDeviceToHost, st));
        BJ_HIP(ctx, hipMemcpyAsync(status.data() + n_oracles * (size_t)chains, DA.status, (size_t)chains * 4, hipMemcpyDeviceToHost, st));
        BJ_HIP(ctx, hipStreamSynchronize(st));
        return BJ_OK;
    };
    auto failure_of = [&](const bj::VerifyBatchProof &r, uint32_t chains) {
        return first_failure(status.data() + r.chain0, chains, status.data() + n_oracles * (size_t)chains + r.chain0, r.nq, G.n_fri);
    };
    if (int rc = launch(D + P.record_table, dev.size(), P.n_chains, true)) return rc;
    T->state = 2;
    std::vector<Failure> at_drawn(dev.size());
    std::vector<size_t> again;   // positions in dev whose verdict needs the stored indices
    for (size_t k = 0; k < dev.size(); k++) {
        at_drawn[k] = failure_of(P.records[k], P.n_chains);
        if (device_verdict(&out[dev[k]], nqs[k], R[dev[k]].first_mismatch, at_drawn[k], nullptr)) again.push_back(k);
    }
    if (again.empty()) return BJ_OK;
    std::vector<bj::VerifyBatchProof> second;
    const uint32_t chains2 = bj::plan_verify_second_pass(P, again, &second);
    BJ_HIP(ctx, hipMemcpyAsync(D + P.record_table2, second.data(), second.size() * sizeof(bj::VerifyBatchProof), hipMemcpyHostToDevice, st));
    if (int rc = launch(D + P.record_table2, second.size(), chains2, false)) return rc;
    for (size_t j = 0; j < again.size(); j++) {
        const size_t k = again[j];
        const Failure at_stored = failure_of(second[j], chains2);
        device_verdict(&out[dev[k]], nqs[k], R[dev[k]].first_mismatch, at_drawn[k], &at_stored);
    }
    return BJ_OK;
}

// bj_verify / bj_verify_proof: the batch path with one proof
int verify_impl(bj_ctx *ctx, const bj_vk *K, const u64 *W, size_t n_words, unsigned flags, bj_verify_report *out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!K || !W || !out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify: null argument");
    if (flags & ~BJ_VERIFY_PARTIAL_QUERIES) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify: unknown flags %#x", flags);
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify: a proof is running on this context");
    std::memset(out, 0, sizeof(*out));
    ctx->verify_timing.state = 0;
    Prepared R;
    if (int rc = prepare(K, W, n_words, flags, &R)) return bj::fail(ctx, rc, "%s", R.err.c_str());
    *out = R.report;
    return judge(ctx, K, &R, 1, out, &ctx->verify_timing);
}

// the key's gates: the shapes of a resolved list, each op-list gate with its packed program from program_of(spec, g, &program)
template <class ProgramOf>
void take_gates(bj_vk *k, const bj::GateList &L, ProgramOf program_of) {
    k->n_gate_terms = L.n_general_terms;
    k->n_spec_terms = L.n_spec_terms;
    for (bool spec : {false, true}) {
        const std::vector<bj::GateShape> &shapes = spec ? L.spec : L.general;
        std::vector<bj_vk::Gate> &to = spec ? k->spec : k->gates;
        to.resize(shapes.size());
        for (size_t g = 0; g < shapes.size(); g++) {
            static_cast<bj::GateShape &>(to[g]) = shapes[g];
            if (shapes[g].kind == BJ_GATE_PROGRAM) program_of(spec, g, &to[g].prog);
        }
    }
}

void finish_config(bj_vk *k, unsigned fri_lde, unsigned security, unsigned pow_bits, unsigned transcript, unsigned hasher, unsigned pow_runner) {
    k->layout = bj::proof_layout(*k);
    k->fri_lde = fri_lde; k->security = security; k->pow_bits = pow_bits;
    k->transcript = transcript ? transcript : BJ_TRANSCRIPT_POSEIDON2;
    k->hasher = hasher ? hasher : BJ_HASHER_POSEIDON2;
    k->pow_runner = pow_runner ? pow_runner : BJ_POW_BLAKE2S256;
}

}  // namespace

extern "C" {

int bj_vk_create(const bj_circuit *c, const uint64_t *setup_cap, const bj_proof_config *cfg, bj_vk **out) {
    if (!out) return bj::fail(nullptr, BJ_ERR_INVALID_ARG, "bj_vk_create: null out pointer");
    *out = nullptr;
    if (!c || !cfg || !setup_cap) return bj::fail(nullptr, BJ_ERR_INVALID_ARG, "bj_vk_create: null argument");
    bj::GateList L;
    if (int rc = bj::circuit_check(nullptr, "bj_vk_create", c, cfg, true, nullptr, &L)) return rc;
    bj_vk *k = new bj_vk();
    static_cast<bj::CircuitShape &>(*k) = bj::circuit_shape(c, cfg);
    auto take_program = [](const bj_gate_program *p, bj_vk::Program *P) {   // circuit_check has canonicalised it once: it cannot fail here
        bj::canon::Program C;
        std::string err;
        if (bj::canon::canonicalize(p, &C, &err)) return;
        bj::pack_program(C, &P->rel, &P->values);
        P->n_slots = C.num_slots;
    };
    take_gates(k, L, [&](bool spec, size_t g, bj_vk::Program *P) { take_program((spec ? c->specialized_gates : c->gates)[g].program, P); });
    k->non_residues.assign(c->non_residues, c->non_residues + c->num_vars);
    for (unsigned i = 0; i < c->num_public_inputs; i++) {
        k->pub_cols.push_back(c->public_input_cols[i]);
        k->pub_rows.push_back(c->public_input_rows[i]);
    }
    finish_config(k, cfg->fri_lde_factor, cfg->security_level, cfg->pow_bits, cfg->transcript, cfg->tree_hasher, cfg->pow_runner);
    k->cap.assign(setup_cap, setup_cap + 4 * (size_t)cfg->cap_size);
    *out = k;
    return BJ_OK;
}

int bj_vk_from_setup(const bj_setup *S, bj_vk **out) {
    if (!out) return bj::fail(nullptr, BJ_ERR_INVALID_ARG, "bj_vk_from_setup: null out pointer");
    *out = nullptr;
    if (!S) return bj::fail(nullptr, BJ_ERR_INVALID_ARG, "bj_vk_from_setup: null setup");
    bj_vk *k = new bj_vk();
    static_cast<bj::CircuitShape &>(*k) = *S;
    auto take_program = [](const bj::DevProgram &d, bj_vk::Program *P) {
        P->rel = d.h_rel;
        P->values = d.h_values;
        P->n_slots = slots_of(P->rel);
    };
    take_gates(k, S->gates, [&](bool spec, size_t g, bj_vk::Program *P) { take_program((spec ? S->spec_programs : S->programs)[g], P); });
    k->non_residues = S->non_residues;
    k->pub_cols = S->pub_cols;
    k->pub_rows = S->pub_rows;
    finish_config(k, S->fri_lde, S->security, S->pow_bits, S->transcript, S->hasher, S->pow_runner);
    k->cap = S->cap;
    *out = k;
    return BJ_OK;
}

void bj_vk_destroy(bj_vk *vk) { delete vk; }

int bj_verify(bj_ctx *ctx, const bj_vk *vk, const uint64_t *proof_words, size_t n_words, unsigned flags, bj_verify_report *out) {
    return verify_impl(ctx, vk, proof_words, n_words, flags, out);
}

int bj_verify_proof(bj_ctx *ctx, const bj_vk *vk, const bj_proof *proof, bj_verify_report *out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_proof: null proof");
    const std::vector<u64> &w = bj::proof_words(proof);
    return verify_impl(ctx, vk, w.data(), w.size(), 0, out);
}

// bj_verify_batch: N proofs of one key — prepare() on worker threads, then the judge over those that got as far
int bj_verify_batch(bj_ctx *ctx, const bj_vk *K, const uint64_t *const *proofs, const size_t *n_words, size_t n_proofs, unsigned flags,
                    bj_verify_report *out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!K) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: null key");
    if (flags & ~BJ_VERIFY_PARTIAL_QUERIES) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: unknown flags %#x", flags);
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: a proof is running on this context");
    if (!n_proofs) return BJ_OK;
    if (!proofs || !n_words || !out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: null argument");
    if (n_proofs > bj::VERIFY_BATCH_MAX_PROOFS)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: %zu proofs in one call, at most %zu", n_proofs, bj::VERIFY_BATCH_MAX_PROOFS);
    for (size_t i = 0; i < n_proofs; i++)
        if (!proofs[i] && n_words[i]) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch: proof %zu is null with %zu words", i, n_words[i]);
    std::memset(out, 0, n_proofs * sizeof(*out));
    VerifyTiming &T = ctx->verify_batch_timing;
    T.state = 0;

    // prepare() of every proof, proofs handed out in order to a bounded pool
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Prepared> R(n_proofs);
    {
        const unsigned limit = bj::env().verify_threads;
        const size_t n_workers = n_proofs < limit ? n_proofs : limit;
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (size_t i; (i = next.fetch_add(1)) < n_proofs;) prepare(K, proofs[i], n_words[i], flags, &R[i]);
        };
        std::vector<std::thread> pool;
        for (size_t w = 1; w < n_workers; w++) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    }
    T.host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t i = 0; i < n_proofs; i++)
        if (R[i].rc) return bj::fail(ctx, R[i].rc, "%s (proof %zu of the batch)", R[i].err.c_str(), i);
    for (size_t i = 0; i < n_proofs; i++) out[i] = R[i].report;
    T.state = 1;
    return judge(ctx, K, R.data(), n_proofs, out, &T);
}

int bj_verify_batch_ms(bj_ctx *ctx, float *host_ms, float *upload_ms, float *openings_ms, float *deep_fri_ms) {
    if (int rc = bj::bind(ctx)) return rc;
    const VerifyTiming &T = ctx->verify_batch_timing;
    if (!T.state) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_batch_ms: no bj_verify_batch has run on this context");
    float up = 0, a = 0, b = 0;
    if (T.state == 2) {   // the batch reached its kernels (it synchronised behind them)
        BJ_HIP(ctx, hipEventElapsedTime(&up, T.ev[0], T.ev[1]));
        BJ_HIP(ctx, hipEventElapsedTime(&a, T.ev[1], T.ev[2]));
        BJ_HIP(ctx, hipEventElapsedTime(&b, T.ev[2], T.ev[3]));
    }
    if (host_ms) *host_ms = T.host_ms;
    if (upload_ms) *upload_ms = up;
    if (openings_ms) *openings_ms = a;
    if (deep_fri_ms) *deep_fri_ms = b;
    return BJ_OK;
}

int bj_verify_kernel_ms(bj_ctx *ctx, float *openings_ms, float *deep_fri_ms) {
    if (int rc = bj::bind(ctx)) return rc;
    const VerifyTiming &T = ctx->verify_timing;
    if (T.state != 2) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_verify_kernel_ms: the last bj_verify on this context did not reach its kernels");
    float a = 0, b = 0;
    BJ_HIP(ctx, hipEventElapsedTime(&a, T.ev[1], T.ev[2]));
    BJ_HIP(ctx, hipEventElapsedTime(&b, T.ev[2], T.ev[3]));
    if (openings_ms) *openings_ms = a;
    if (deep_fri_ms) *deep_fri_ms = b;
    return BJ_OK;
}

}  // extern "C"
