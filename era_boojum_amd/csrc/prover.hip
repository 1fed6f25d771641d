// Whole-prover orchestration: bj_prove_dev / bj_prove (seam S1 of SURVEY.md §8b) over a setup made by setup.hip, on one GPU
// or with the LDE cosets of one proof split across several (bj_comm, include/boojum_hip.h).
// Follows prove_cpu_basic (src/cs/implementations/prover.rs:153-2266) round by round; the host only runs the
// Fiat–Shamir transcript and O(#columns) scalar arithmetic, every polynomial stays in HBM.
//
// Circuit class: general-purpose gates ConstantsAllocator / FMA-without-constant / Reduction<4> / Nop selected by a
// selector tree over the first constant columns, specialized lookups with a shared constant table id
// (LookupParameters::UseSpecializedColumnsWithTableIdAsConstant) or no lookups, no witness columns, Poseidon2 tree
// hasher + Poseidon2 transcript, PoW off — the configuration of the reference's SHA-256 bench
// (src/gadgets/sha256/mod.rs:284-375).
#include "ctx.h"
#include "../../include/boojum_hip_diag.h"
#include "async_admission.h"
#include "host_transcript.hpp"
#include "fri_types.h"
#include "gate_program.h"
#include "setup.h"
#include "witness_plan.h"
#include "workspace_plan.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

using gl::u64;

struct bj_proof {
    std::vector<u64> data;
    float stage_ms[8] = {0};
    float comm_ms = 0;             // sharded proofs: time between the start and the end of every collective on this rank, summed
    unsigned comm_calls = 0;
    size_t comm_bytes = 0;         // bytes received from the other ranks
    size_t ws_reserved = 0, ws_high_water = 0, ws_overflow_slabs = 0;   // bj_proof_workspace_bytes
    struct KernelStat {            // bj_proof_kernel_stats: first launch of each probed kernel
        const char *name;
        float ms;
        double bytes;
    } kernel_stats[BJ_MAX_KERNEL_PROBES] = {};
    unsigned n_kernel_stats = 0;
};

namespace {

gl::e2 e2c(const u64 *p) { return {gl::canon(p[0]), gl::canon(p[1])}; }

struct StageTimer {
    hipStream_t s;
    std::chrono::steady_clock::time_point t0;
    explicit StageTimer(hipStream_t st) : s(st) {
        (void)hipStreamSynchronize(s);
        t0 = std::chrono::steady_clock::now();
    }
    float lap() {
        (void)hipStreamSynchronize(s);
        auto t1 = std::chrono::steady_clock::now();
        float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};


}  // namespace

namespace bj {
const std::vector<u64> &proof_words(const bj_proof *p) { return p->data; }   // bj_verify_proof (verifier.hip)
int all_gather(bj_ctx *ctx, const Shard &sh, const u64 *d_send, u64 *d_recv, size_t elems) {
    if (!elems) return BJ_OK;
    if (sh.world == 1) {
        if (d_send != d_recv)
            BJ_HIP(ctx, hipMemcpyAsync(d_recv, d_send, elems * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return BJ_OK;
    }
    ctx->comm_bytes += elems * 8 * (sh.world - 1);
    if (sh.comm.all_gather_stream) {   // stream-ordered transport (in-library RCCL): no synchronisation on either side
        hipEvent_t *ev = nullptr;
        if (ctx->in_proof && ctx->comm_n < 48) {
            ev = ctx->comm_ev[ctx->comm_n];
            (void)ensure_event(ctx, ev[0]);   // without its events a collective is not timed, and runs all the same
            (void)ensure_event(ctx, ev[1]);
            if (ev[0] && ev[1]) (void)hipEventRecord(ev[0], ctx->stream);
        }
        if (int rc = sh.comm.all_gather_stream(sh.comm.user, d_send, d_recv, elems * 8, ctx->stream))
            return fail(ctx, BJ_ERR_HIP, "sharded prover: the stream-ordered all_gather failed (%d)", rc);
        if (ev && ev[0] && ev[1]) {
            (void)hipEventRecord(ev[1], ctx->stream);
            ctx->comm_n++;
        }
        return BJ_OK;
    }
    if (!sh.comm.all_gather) return fail(ctx, BJ_ERR_INVALID_ARG, "sharded prover: no all_gather callback");
    BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = sh.comm.all_gather(sh.comm.user, d_send, d_recv, elems * 8))
        return fail(ctx, BJ_ERR_HIP, "sharded prover: the host's all_gather callback failed (%d)", rc);
    ctx->comm_host_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ctx->in_proof) ctx->comm_n += 0x10000;   // high half: synchronous calls
    return BJ_OK;
}

int all_gather_columns(bj_ctx *ctx, const Shard &sh, const u64 *d_send, u64 *d_dst, unsigned parts, size_t part_len) {
    if (sh.world == 1) return all_gather(ctx, sh, d_send, d_dst, (size_t)parts * part_len);
    const size_t per = (size_t)parts * part_len;
    TmpBuf staging;
    if (int rc = staging.alloc(ctx, gather_columns_staging_words(sh.world, parts, part_len))) return rc;
    const u64 *tmp = staging.p;
    int rc = all_gather(ctx, sh, d_send, staging.p, per);
    if (!rc) {
        // tmp[r][p][part_len] -> dst[p][r][part_len]: for each rank one strided 2-D copy
        for (unsigned r = 0; r < sh.world && !rc; r++)
            if (hipMemcpy2DAsync(d_dst + (size_t)r * part_len, (size_t)sh.world * part_len * 8, tmp + (size_t)r * per,
                                 part_len * 8, part_len * 8, parts, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
                rc = fail(ctx, BJ_ERR_HIP, "all_gather_columns: device copy failed");
        (void)hipStreamSynchronize(ctx->stream);
    }
    return rc;
}

int gather_cap(bj_ctx *ctx, const Shard &sh, const u64 *d_tree_local, size_t leaves_local, size_t cap_size, u64 *h_cap) {
    const size_t cap_l = cap_size / sh.world;
    if (sh.world == 1) return bj_merkle_tree_cap(ctx, d_tree_local, leaves_local, cap_size, h_cap);
    // the local cap fragment is the last layer of the local subtree
    const u64 *frag = d_tree_local + (2 * leaves_local - 2 * cap_l) * 4;
    u64 *d_all = gather_area(ctx);
    if (cap_size * 4 > SmallBlock::GATHER_WORDS) return fail(ctx, BJ_ERR_INVALID_ARG, "gather_cap: cap too large");
    if (int rc = all_gather(ctx, sh, frag, d_all, cap_l * 4)) return rc;
    return bj_memcpy_d2h(ctx, h_cap, d_all, cap_size * 32);
}
}  // namespace bj

extern "C" {

void bj_proof_destroy(bj_proof *p) { delete p; }
size_t bj_proof_size_u64(const bj_proof *p) { return p ? p->data.size() : 0; }
int bj_proof_serialize(const bj_proof *p, uint64_t *out) {
    if (!p || !out) return BJ_ERR_INVALID_ARG;
    std::memcpy(out, p->data.data(), p->data.size() * 8);
    return BJ_OK;
}
int bj_proof_comm_stats(const bj_proof *p, float *ms_in_collectives, size_t *calls, size_t *bytes_received) {
    if (!p) return BJ_ERR_INVALID_ARG;
    if (ms_in_collectives) *ms_in_collectives = p->comm_ms;
    if (calls) *calls = p->comm_calls;
    if (bytes_received) *bytes_received = p->comm_bytes;
    return BJ_OK;
}
int bj_proof_kernel_stats(const bj_proof *p, unsigned index, const char **name, float *ms, double *algorithmic_bytes) {
    if (!p || index >= p->n_kernel_stats) return BJ_ERR_INVALID_ARG;
    if (name) *name = p->kernel_stats[index].name;
    if (ms) *ms = p->kernel_stats[index].ms;
    if (algorithmic_bytes) *algorithmic_bytes = p->kernel_stats[index].bytes;
    return BJ_OK;
}
int bj_proof_workspace_bytes(const bj_proof *p, size_t *reserved, size_t *high_water, size_t *overflow_slabs) {
    if (!p) return BJ_ERR_INVALID_ARG;
    if (reserved) *reserved = p->ws_reserved;
    if (high_water) *high_water = p->ws_high_water;
    if (overflow_slabs) *overflow_slabs = p->ws_overflow_slabs;
    return BJ_OK;
}
int bj_proof_stage_ms(const bj_proof *p, float *out8) {
    if (!p || !out8) return BJ_ERR_INVALID_ARG;
    std::memcpy(out8, p->stage_ms, sizeof(p->stage_ms));
    return BJ_OK;
}

}  // extern "C"

namespace {
// bj_prove: the witness is still in host memory when the proof starts.  Its columns are copied in groups on a second stream,
// every group followed by an event; the witness round below waits for a group right before it transforms it, so the PCIe
// transfer of the later groups runs under the iNTT / LDE of the earlier ones (the host buffers should be pinned).
struct HostWitness {
    const uint64_t *h_variables, *h_multiplicities;
    unsigned group;        // columns per group
    bool no_absorb;        // transfer and transform in groups, hash once at the end (a lane of bj_prove_async whose sibling is proving)
};
// bj_prove_values: the host holds a WitnessVec (witness.rs:29-71), not columns.  all_values crosses PCIe once, on the copy stream,
// into the witness staging behind the multiplicity column, the u32 counters behind it; the columns of every group are then gathered
// on the proof stream through the setup's resident placements (witness_gather_kernel) into the staging the host path copies into,
// and everything below "how a group's columns arrive" is the host path's.
struct ValuesWitness {
    const uint64_t *h_values;
    size_t n_values;
    const uint32_t *h_multiplicities;   // nullptr: counted on the device
    size_t n_multiplicities;
    uint64_t *d_values;                 // [n_values] in the staging
    uint32_t *d_counters;               // [n] u32 behind them
    unsigned group;
    bool no_absorb;
};

using Src = bj::OpenSrc;   // opening_args.h: a base-field column (c1 == nullptr) or the two columns of an F_p^2 polynomial
struct DeepSets;
struct Queries;

// A proof in the making: what lives from one round to the next, and the rounds in the order prove_impl runs them.  Each says
// above its definition what it reads from this object and what it adds to it.  Arena buffers are never given back (bump
// allocator): the order of the takes IS the layout of the workspace, and `plan` (workspace_plan.h) is that order written down.
struct Proving {
    bj_ctx *ctx;
    const bj_setup *S;
    const bj::Shard &sh;
    hipStream_t st;
    const u64 *d_variables, *d_multiplicities, *h_public_values;
    const HostWitness *hw;   // nullptr: the witness is resident (bj_prove_dev) ...
    const ValuesWitness *vw = nullptr;   // ... or comes as values (bj_prove_values); never both
    bool values_unchecked = false;       // gathers have been launched and their flag has not been read yet (check_values_flag)
    const bj::ProofLayout &L;   // proof_layout.h: the columns of every oracle, the opening order, the proof's words
    bool has_lookup;
    bool count_mult;         // no multiplicity column was supplied: round 1 counts it (count_multiplicities)
    bool absorb;             // staged witness: the leaves absorb every column group as it lands (witness_from_host)
    unsigned log_n, V, q;
    // N / Ln: leaves / column stride HELD BY THIS GPU (the whole domain on one GPU); Q: points of the quotient domain
    size_t n, N, Q, Ln, I0, capl;
    // quotient evaluation: the q n points are split evenly, rank r evaluates on the first Qe = q n / W points of ITS OWN range of
    // the LDE (they form the coset x_{I0} * H_Qe in bit-reversed order, whether Qe is several cosets of H_n, one, or a fraction
    // of one), inverse-transforms them to T mod (x^Qe - x_{I0}^Qe), and the residues are all-gathered and combined (round 3)
    size_t Qe;            // points this rank evaluates
    unsigned VW;          // variables, then the non-copiable witness columns (prover.rs:317-343): the columns in front of the multiplicities
    unsigned nW, nS2;     // leaf widths of the witness and the stage-2 oracle
    bj_proof *proof = nullptr;
    bj::host::Transcript tr;
    u64 beta[2], gamma[2], lbeta[2] = {0, 0}, lgamma[2] = {0, 0}, z[2], zo[2];   // challenges of rounds 2 and 4 (zo = z * omega)
    bj::WorkspacePlan plan;
    // The four committed oracles (oracle_value.h) by ORACLE_*: width, stride and residency from the constructor, the pointers as the
    // rounds take the buffers below.  The setup's is S's own; a lean one gets setup_coset for its evaluations in round 3.  After
    // round 3 the coset buffer of a lean oracle holds coset 0, which round 4 evaluates from.
    bj::Oracle oracle[4];
    bj::TmpBuf wit_lde, wit_tree, mono, mono_s2;   // mono: witness monomials, mono_s2: stage-2 monomials (both kept for DEEP)
    bj::TmpBuf s2_lde, s2_tree, T, q_lde, q_tree, deep, setup_coset;
    std::vector<u64> wit_cap, s2_cap, q_cap;
    std::vector<u64> vz, vzo, v0;   // the opened values
    uint32_t sched[32];             // FRI folding schedule (bj_fri_schedule, before the workspace is reserved)
    uint32_t new_pow = 0;           // proof-of-work bits left once the query count is rounded
    size_t sched_len = 0, num_queries = 0, final_degree = 0;
    bj_fri *fri = nullptr;
    u64 pow_challenge = 0;

    // the witness columns arrive in the context's staging group by group: copied from the host, or gathered from values
    bool staged() const { return hw || vw; }
    unsigned staged_group() const { return hw ? hw->group : vw->group; }
    Proving(bj_ctx *c, const bj_setup *s, const u64 *d_vars, const u64 *d_mult, const u64 *h_pub, const HostWitness *h, const ValuesWitness *v,
            bool count)
        : ctx(c), S(s), sh(s->sh), st(c->stream), d_variables(d_vars), d_multiplicities(d_mult), h_public_values(h_pub), hw(h), vw(v), L(s->layout) {
        has_lookup = L.has_lookup;
        count_mult = has_lookup && count;
        log_n = S->log_n, V = S->V, q = S->q;
        n = (size_t)1 << log_n, N = S->Nl, Q = n * q, Ln = S->Ls, I0 = (size_t)S->c0 * n, capl = S->cap_l;
        Qe = Q / sh.world;
        VW = L.multiplicity();
        nW = L.widths[bj::ORACLE_WITNESS], nS2 = L.widths[bj::ORACLE_STAGE2];
        // BJ_PROOF_LEAN, or the lane of bj_prove_async that admitted this proof with a lean workspace (ctx.h: lean_override): the
        // witness and stage-2 oracles keep no evaluations
        const bool lean_p = (c->lean_override >= 0 ? c->lean_override != 0 : bj::env().proof_lean) && sh.world == 1;
        oracle[bj::ORACLE_WITNESS] = bj::oracle_of(nW, n, Ln, !lean_p);
        oracle[bj::ORACLE_STAGE2] = bj::oracle_of(nS2, n, Ln, !lean_p);
        oracle[bj::ORACLE_QUOTIENT] = bj::oracle_of(2 * q, n, N, true);   // always resident, on the FRI domain; its monomials: T's chunk layout
        oracle[bj::ORACLE_QUOTIENT].mono_parts = 2, oracle[bj::ORACLE_QUOTIENT].mono_part_gap = Q;
        oracle[bj::ORACLE_SETUP] = S->oracle();
        absorb = staged() && (S->hasher == BJ_HASHER_POSEIDON2 || S->hasher == BJ_HASHER_POSEIDON) && !bj::env().prove_no_absorb &&
                 !(hw ? hw->no_absorb : vw->no_absorb) && oracle[bj::ORACLE_WITNESS].resident;
    }
    int reserve_workspace();
    int check_public_inputs();
    int open_transcript();
    int count_multiplicities();
    int round1_witness();
    int witness_from_host();
    int queue_host_copies(const std::vector<bj::WitnessGroup> &plan);
    int queue_values_upload();
    int gather_columns(unsigned c0, unsigned c1);
    int check_values_flag();
    int round2_stage2();
    int round3_quotient();
    int exchange_residues(u64 *Tl);
    enum Brought { MONOMIALS, EXTENDED, LEAVES_HASHED };   // how far its round has brought a resident oracle when it is committed
    int commit(const bj::Oracle &o, std::vector<u64> &cap, Brought have, float *leaf_ms = nullptr);
    int round4_openings();
    std::vector<Src> sources(const std::vector<bj::Opened> &polys, bool on_evals) const;
    int evaluate_at(u64 *w, u64 open_shift, const std::vector<Src> &ss, const u64 *at, std::vector<u64> &vals);
    int round5a_deep();
    int deep_set(DeepSets &D, const std::vector<bj::Opened> &polys, const u64 *vals, const u64 *at);
    int flush_deep(DeepSets &D);
    int round5b_fri();
    int round6_queries(Queries &qr);
    int gather_base_queries(Queries &qr);
    int gather_fri_queries(Queries &qr);
    int serialise(const Queries &qr);
    void read_back_stats();

    void challenge2(u64 *o) {
        o[0] = tr.challenge();
        o[1] = tr.challenge();
    }
    // inverse transform of columns of the main domain into the monomial layout of this trace length; extension out of it
    int intt_cols(const u64 *d_in, u64 *d_out, unsigned nc) const {
        return S->tiled ? bj::intt_to_tiled(ctx, d_in, n, d_out, n, log_n, nc) : bj_intt_batch(ctx, d_in, d_out, log_n, nc, n, 1);
    }
    int lde_cols(const u64 *d_m, u64 *d_out, size_t out_stride, unsigned nc, unsigned log_lde, unsigned cb, unsigned cc) const {
        return bj::lde_cosets_strided(ctx, d_m, n, d_out, out_stride, log_n, nc, log_lde, cb, cc, S->tiled);
    }
    // a lean oracle's coset buffer is made to hold coset c; a resident oracle has every coset
    int rebuild(const bj::Oracle &o, unsigned c) const { return o.resident ? BJ_OK : lde_cols(o.mono, o.evals, o.stride, o.width, S->log_L, c, 1); }
};

// 1, x, x^2, ... as F_p^2 pairs (materialize_powers_serial, utils.rs:31; materialize_ext_challenge_powers, prover.rs:2374-2395)
std::vector<u64> e2_powers(const u64 *x, size_t count) {
    std::vector<u64> out(2 * count);
    gl::e2 a = e2c(x), cur{1, 0};
    for (size_t i = 0; i < count; i++) {
        out[2 * i] = cur.c0;
        out[2 * i + 1] = cur.c1;
        cur = gl::e2_mul(cur, a);
    }
    return out;
}

// The shape of the workspace (workspace_plan.h) of a proof of S: from the setup, how the witness arrives, whether the witness and
// stage-2 oracles keep their evaluations, and the FRI schedule.  One function behind the reservation of a proof and the admission
// of bj_prove_async, which asks before a proof exists.
bj::WorkspaceShape shape_of(const bj_setup *S, bool mult_in_arena, unsigned host_witness, bool lean_oracles, uint32_t new_pow, const uint32_t *sched,
                            size_t sched_len, size_t num_queries) {
    const bj::ProofLayout &L = S->layout;
    const unsigned alpha_terms = L.n_lookup_terms + S->gates.n_spec_terms + S->gates.n_general_terms + 1 + L.n_chunks;
    bj::WorkspaceShape shape = bj::workspace_shape(L, S->sh.world, S->tiled, alpha_terms, S->pub_cols.data(), S->pub_rows.data(), S->pub_cols.size(),
                                                   mult_in_arena, host_witness, new_pow != 0, sched, sched_len, num_queries);
    shape.lean = !S->oracle().resident;
    shape.lean_oracles = lean_oracles;
    return shape;
}

// Reads the setup's parameters and the sizes.  Adds the FRI schedule and the workspace plan; resets the context's arena to one
// reservation for every buffer of the proof (a context that has seen a larger proof keeps its size); adds proof->ws_reserved.
int Proving::reserve_workspace() {
    if (int rc = bj_fri_schedule(S->security, S->cap_size, S->pow_bits, S->log_fri, log_n, &new_pow, &num_queries, sched, &sched_len, &final_degree))
        return bj::fail(ctx, rc, "bj_prove: compute_fri_schedule failed");
    plan = bj::workspace_plan(shape_of(S, count_mult && !d_multiplicities,
                                       !staged() ? bj::WS_HOST_NONE : absorb ? bj::WS_HOST_ABSORBING : bj::WS_HOST_NOT_ABSORBING,
                                       !oracle[bj::ORACLE_WITNESS].resident, new_pow, sched, sched_len, num_queries));
    if (int rc = bj::arena_reset(ctx, std::max(plan.total(), ctx->arena_learned))) return rc;
    proof->ws_reserved = ctx->bump.arena_words * 8;
    return BJ_OK;
}

// Reads the witness cells the public inputs name (from the host witness, or off the device: one synchronisation of the stream).
// The values that go into the transcript must be the cells they claim to be (witness.rs:21-27).
int Proving::check_public_inputs() {
    if (S->pub_cols.empty() || vw) return BJ_OK;   // from values: the public values were read through the placement, they ARE the cells
    std::vector<u64> cells(S->pub_cols.size());
    for (size_t i = 0; i < cells.size(); i++) {
        const size_t at = (size_t)S->pub_cols[i] * n + S->pub_rows[i];
        if (hw)
            cells[i] = hw->h_variables[at];
        else
            BJ_HIP(ctx, hipMemcpyAsync(&cells[i], d_variables + at, 8, hipMemcpyDeviceToHost, st));
    }
    if (!hw) BJ_HIP(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < cells.size(); i++)
        if (gl::canon(cells[i]) != gl::canon(h_public_values[i]))
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove: public input %zu: value %llu given, the witness holds %llu at (column %u, row %u)",
                            i, (unsigned long long)gl::canon(h_public_values[i]), (unsigned long long)gl::canon(cells[i]),
                            S->pub_cols[i], S->pub_rows[i]);
    return BJ_OK;
}

// Starts the transcript with the setup cap and the public inputs; makes sure the twiddles of the LDE domain exist.
int Proving::open_transcript() {
    tr.kind = (int)S->transcript;
    tr.absorb_cap(S->cap.data(), S->cap.size());                                   // prover.rs:211
    if (!S->pub_cols.empty()) tr.absorb(h_public_values, S->pub_cols.size());   // prover.rs:257-259
    return bj::ensure_twiddles(ctx, log_n + (S->L > S->fri_lde ? bj::log2_exact(S->L) : S->log_fri), false);
}

// A host witness: the copies of every column group are queued on the copy stream at once, each followed by its event.
int Proving::queue_host_copies(const std::vector<bj::WitnessGroup> &plan) {
    for (unsigned g = 0; g < (unsigned)plan.size(); g++) {
        if (int rc = bj::ensure_event(ctx, ctx->copy_ev[g], hipEventDisableTiming)) return rc;
        const unsigned c0 = plan[g].c0, c1 = plan[g].c1;
        const unsigned v1 = c1 < VW ? c1 : VW;         // variable / witness columns of this group: [c0, v1)
        if (c0 < v1)
            BJ_HIP(ctx, hipMemcpyAsync(const_cast<uint64_t *>(d_variables) + (size_t)c0 * n, hw->h_variables + (size_t)c0 * n,
                                       (size_t)(v1 - c0) * n * 8, hipMemcpyHostToDevice, ctx->copy_stream));
        if (has_lookup && !count_mult && c1 == nW)
            BJ_HIP(ctx, hipMemcpyAsync(const_cast<uint64_t *>(d_multiplicities), hw->h_multiplicities, n * 8, hipMemcpyHostToDevice,
                                       ctx->copy_stream));
        BJ_HIP(ctx, hipEventRecord(ctx->copy_ev[g], ctx->copy_stream));
    }
    return BJ_OK;
}

// Values: all_values goes up once on the copy stream, followed by event 0; the u32 counters go up behind it, followed by event 1.
// The gather's flag is cleared on the proof stream, in front of the first gather.
int Proving::queue_values_upload() {
    for (unsigned e = 0; e < 2; e++)
        if (int rc = bj::ensure_event(ctx, ctx->copy_ev[e], hipEventDisableTiming)) return rc;
    if (vw->n_values)
        BJ_HIP(ctx, hipMemcpyAsync(vw->d_values, vw->h_values, vw->n_values * 8, hipMemcpyHostToDevice, ctx->copy_stream));
    BJ_HIP(ctx, hipEventRecord(ctx->copy_ev[0], ctx->copy_stream));
    if (has_lookup && !count_mult && vw->n_multiplicities)
        BJ_HIP(ctx, hipMemcpyAsync(vw->d_counters, vw->h_multiplicities, vw->n_multiplicities * 4, hipMemcpyHostToDevice, ctx->copy_stream));
    BJ_HIP(ctx, hipEventRecord(ctx->copy_ev[1], ctx->copy_stream));
    BJ_HIP(ctx, hipMemsetAsync(bj::values_bad_flag(ctx), 0, 4, st));
    return BJ_OK;
}

// Columns [c0, c1) of the witness (variables, then the non-copiable witness columns) gathered from the values through the setup's
// placements, straight into the staging a host witness is copied into.
int Proving::gather_columns(unsigned c0, unsigned c1) {
    u64 *cells = const_cast<u64 *>(d_variables);
    const unsigned ve = c1 < V ? c1 : V, wb = c0 > V ? c0 : V;   // [c0, ve): variable columns; [wb, c1): witness columns
    if (c0 < ve)
        bj::launch_witness_gather(S->d_placement + (size_t)c0 * n, vw->d_values, vw->n_values, cells + (size_t)c0 * n, (size_t)(ve - c0) * n,
                                  bj::values_bad_flag(ctx), st);
    if (wb < c1)
        bj::launch_witness_gather(S->d_wit_placement + (size_t)(wb - V) * n, vw->d_values, vw->n_values, cells + (size_t)wb * n,
                                  (size_t)(c1 - wb) * n, bj::values_bad_flag(ctx), st);
    BJ_CHECK_LAUNCH(ctx);
    values_unchecked = true;
    return BJ_OK;
}

// Reads the gather's flag (synchronises; called where round 1 synchronises anyway): a cell that named a value at or beyond n_values
// refuses the proof.  Nothing to do for any other witness source, or once the flag has been read after the last gather.
int Proving::check_values_flag() {
    if (!values_unchecked) return BJ_OK;
    unsigned bad = 0;
    if (int rc = bj_memcpy_d2h(ctx, &bad, bj::values_bad_flag(ctx), 4)) return rc;
    values_unchecked = false;
    if (bad) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_values: a cell names a variable beyond all_values");
    return BJ_OK;
}

// Round 1 with the witness staged group by group (hw: copied from host memory; vw: gathered from values): walks the plan of
// column groups, transforms each group on the proof stream as it arrives.  Reads mono, wit_lde, wit_tree (allocated); fills mono
// and, the oracle resident, wit_lde.  absorb: the leaves are absorbed group by group as well, and the leaf layer of wit_tree is
// written here.
int Proving::witness_from_host() {
    int rc = BJ_OK;
    const bj::Oracle &wit = oracle[bj::ORACLE_WITNESS];
    // all copies are queued on the copy stream at once (they run back to back at PCIe speed); the proof stream picks the
    // groups up as they land.  Column nW - 1 is the multiplicity column when there are lookups.
    if (!ctx->copy_stream) BJ_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    // groups of G columns, at most 64 of them (one event each): a wide witness gets wider groups instead of an error.  With
    // an algebraic tree hasher (Poseidon2 / Poseidon) and G a multiple of the sponge's rate, a group is also absorbed into the leaf sponges as soon
    // as it is extended (the capacity words of every leaf wait in HBM between the groups), so that hashing — the dominant
    // kernel — runs under the transfer of the later groups instead of after the last one has landed.
    unsigned G = staged_group();
    if ((nW + G - 1) / G > 64) G = (nW + 63) / 64;
    if (absorb) G = (G + 7) / 8 * 8;
    const std::vector<bj::WitnessGroup> plan = bj::host_witness_plan(nW, G, absorb, bj::env().prove_uniform_groups);
    const unsigned n_groups = (unsigned)plan.size();
    bj::TmpBuf capacity;
    if (absorb && (rc = capacity.take(ctx, bj::WS_CAPACITY))) return rc;
    if ((rc = hw ? queue_host_copies(plan) : queue_values_upload())) return rc;
    if (absorb) BJ_HIP(ctx, hipEventRecord(ctx->ev0, st));
    for (unsigned g = 0; g < n_groups && !rc; g++) {
        const unsigned c0 = plan[g].c0, c1 = plan[g].c1;
        const unsigned v1 = c1 < VW ? c1 : VW;
        // how the group's columns arrive: a host witness group by group over PCIe, each behind its event; values once, behind the
        // first event, and from then on every group is a gather on this stream that waits for nothing
        if (hw) {
            BJ_HIP(ctx, hipStreamWaitEvent(st, ctx->copy_ev[g], 0));
        } else {
            if (g == 0) BJ_HIP(ctx, hipStreamWaitEvent(st, ctx->copy_ev[0], 0));
            if (c0 < v1 && (rc = gather_columns(c0, v1))) break;
            if (c1 == nW && has_lookup) {
                if (count_mult) {
                    rc = check_values_flag();   // the count synchronises anyway, and must not name a tuple that a refused cell made
                } else {
                    BJ_HIP(ctx, hipStreamWaitEvent(st, ctx->copy_ev[1], 0));   // the counters went up behind the values
                    bj::launch_widen_counters(vw->d_counters, vw->n_multiplicities, const_cast<u64 *>(d_multiplicities), n, st);
                    BJ_CHECK_LAUNCH(ctx);
                }
                if (rc) break;
            }
        }
        if (count_mult && c1 == nW && (rc = count_multiplicities())) break;   // the last group: every lookup column has landed
        if (c0 < v1) rc = intt_cols(d_variables + (size_t)c0 * n, mono.p + (size_t)c0 * n, v1 - c0);
        if (!rc && has_lookup && c1 == nW) rc = intt_cols(d_multiplicities, mono.p + (size_t)L.multiplicity() * n, 1);
        if (!rc && wit.resident) rc = lde_cols(mono.p + (size_t)c0 * n, wit_lde.p + (size_t)c0 * Ln, Ln, c1 - c0, S->log_L, S->c0, S->cl);
        if (absorb && !rc && plan[g].absorb_from != bj::NO_ABSORB) {
            const unsigned a0 = plan[g].absorb_from;
            bj::launch_tree_leaves_absorb(ctx->hasher, wit_lde.p + (size_t)a0 * Ln, Ln, c1 - a0, N, capacity.p, wit_tree.p, a0 == 0,
                                          c1 == nW, st);
        }
    }
    if (absorb) BJ_HIP(ctx, hipEventRecord(ctx->ev1, st));
    return rc;
}

// No multiplicity column came with the witness: it is counted from the setup's table columns and the lookup columns of the
// variables (lookup_multiplicities.hip), into the witness staging behind the variables where the witness came from the host, into
// a column of the arena otherwise.  Synchronises (the number of misses is read); a tuple that is in no table row ends the proof.
// Reads d_variables; sets d_multiplicities where it was nullptr.
int Proving::count_multiplicities() {
    if (!d_multiplicities) {
        bj::TmpBuf col;
        if (int rc = col.take(ctx, bj::WS_MULTIPLICITY)) return rc;
        d_multiplicities = col.p;
    }
    return bj::setup_lookup_multiplicities(ctx, vw ? "bj_prove_values" : hw ? "bj_prove" : "bj_prove_dev", S, d_variables,
                                           const_cast<u64 *>(d_multiplicities));
}

// Commits to an oracle whose monomials stand: the leaves of its tree over this rank's N points of the FRI domain, the node layers,
// the cap into `cap` and into the transcript.  A resident oracle is extended first (have == MONOMIALS; a round that extends in its
// own way, or has hashed the leaves as well, says so) and its leaves are hashed in one launch.  A lean one is extended one coset
// at a time into its [width][n] buffer, the n leaves of the coset hashed before the next one overwrites it: leaf i of the tree is
// row i of the LDE ([column][coset][n]), so coset c's leaves are the digests [c n, (c + 1) n) of the leaf layer, which is the first
// layer of the tree, 4 c n words in.  The buffer is left holding the last coset.
// leaf_ms: the leaf work is bracketed by HIP events on the launch stream and its time stored there: the leaf kernel alone
// (resident), the coset loop with its transforms and the node layers (lean), what the caller bracketed itself (LEAVES_HASHED).
int Proving::commit(const bj::Oracle &o, std::vector<u64> &cap, Brought have, float *leaf_ms) {
    const bool timed = leaf_ms && have != LEAVES_HASHED;
    if (o.resident) {
        if (have == MONOMIALS)
            if (int rc = lde_cols(o.mono, o.evals, o.stride, o.width, S->log_L, S->c0, S->cl)) return rc;
        if (timed) BJ_HIP(ctx, hipEventRecord(ctx->ev0, st));
        if (have != LEAVES_HASHED) bj::launch_tree_leaves(ctx->hasher, o.evals, o.stride, nullptr, o.width, N, o.tree, st);
        if (timed) BJ_HIP(ctx, hipEventRecord(ctx->ev1, st));
    } else {
        if (timed) BJ_HIP(ctx, hipEventRecord(ctx->ev0, st));
        for (unsigned c = 0; c < (unsigned)(N / n); c++) {
            if (int rc = rebuild(o, c)) return rc;
            bj::launch_tree_leaves(ctx->hasher, o.evals, o.stride, nullptr, o.width, n, o.tree + 4 * (size_t)c * n, st);
        }
    }
    bj::launch_tree_node_layers(ctx->hasher, o.tree, N, capl, st);
    BJ_CHECK_LAUNCH(ctx);
    if (timed && !o.resident) BJ_HIP(ctx, hipEventRecord(ctx->ev1, st));
    cap.resize(4 * S->cap_size);
    if (int rc = bj::gather_cap(ctx, sh, o.tree, N, S->cap_size, cap.data())) return rc;
    if (leaf_ms) BJ_HIP(ctx, hipEventElapsedTime(leaf_ms, ctx->ev0, ctx->ev1));
    if (int rc = check_values_flag()) return rc;   // the stream has drained for the cap: no cap of a witness with a bad cell is absorbed
    tr.absorb_cap(cap.data(), cap.size());
    return BJ_OK;
}

// ---------------- round 1: witness LDE + tree (prover.rs:270-353) ----------------
// Reads d_variables, d_multiplicities (hw: the host witness).  Adds wit_lde, mono, mono_s2 (allocated only), wit_tree, wit_cap;
// the transcript absorbs wit_cap; proof->stage_ms[7] is the time of the leaf work (commit; with a host witness hashed in groups
// the bracket spans the groups' transforms too: the roofline figure comes from bj_prove_dev).
int Proving::round1_witness() {
    int rc = BJ_OK;
    bj::Oracle &wit = oracle[bj::ORACLE_WITNESS];
    if (count_mult && !staged() && (rc = count_multiplicities())) return rc;   // before any proof work
    if ((rc = wit_lde.take(ctx, bj::WS_WIT_LDE))) return rc;
    if ((rc = mono.take(ctx, bj::WS_MONO))) return rc;
    if ((rc = mono_s2.take(ctx, bj::WS_MONO_S2))) return rc;
    if ((rc = wit_tree.take(ctx, bj::WS_WIT_TREE))) return rc;
    wit.mono = mono.p, wit.evals = wit_lde.p, wit.tree = wit_tree.p;
    if (!staged()) {
        rc = intt_cols(d_variables, mono.p, VW);
        if (!rc && has_lookup) rc = intt_cols(d_multiplicities, mono.p + (size_t)L.multiplicity() * n, 1);
    } else {
        rc = witness_from_host();   // a resident oracle is extended there, group by group (a lean one: after the last group has landed)
    }
    if (rc) return rc;
    return commit(wit, wit_cap, !staged() ? MONOMIALS : absorb ? LEAVES_HASHED : EXTENDED, &proof->stage_ms[7]);
}

// ---------------- round 2: copy-permutation + lookup polys (prover.rs:360-554) ----------------
// Reads d_variables, d_multiplicities, the setup's natural-order columns.  Draws beta, gamma (lbeta, lgamma with lookups); fills
// mono_s2; adds s2_lde, s2_tree, s2_cap; the transcript absorbs s2_cap.
int Proving::round2_stage2() {
    int rc = BJ_OK;
    challenge2(beta);
    challenge2(gamma);
    bj::TmpBuf s2_nat, tmp;
    if ((rc = s2_nat.take(ctx, bj::WS_S2_NAT))) return rc;
    if ((rc = tmp.take(ctx, bj::WS_S2_SCRATCH))) return rc;
    const bj::Cols vars{d_variables, n}, nat{S->d_nat, n};
    bj::launch_copy_perm_stage2(bj::CopyPermArg{vars, nat.at(L.sigma(0)), S->d_non_res, V, q, log_n, ctx->tw_fwd.p, beta, gamma, S->small_non_residues},
                                tmp.p, s2_nat.p + (size_t)L.z() * n, s2_nat.p + (size_t)L.partial(0) * n, st);
    if (has_lookup) {
        challenge2(lbeta);
        challenge2(lgamma);
        bj::launch_lookup_polys(bj::LookupArg{vars.at(L.lookup_var(0, 0)), nat.at(L.table(0)), S->tid_var ? nullptr : nat.at(L.table_id()).p,
                                              d_multiplicities, S->lookup_reps, S->lookup_w, lbeta, lgamma},
                                log_n, s2_nat.p + (size_t)L.lookup_a(0) * n, s2_nat.p + (size_t)L.lookup_b() * n, st);
    }
    BJ_CHECK_LAUNCH(ctx);
    if ((rc = s2_lde.take(ctx, bj::WS_S2_LDE))) return rc;
    if ((rc = s2_tree.take(ctx, bj::WS_S2_TREE))) return rc;
    bj::Oracle &s2 = oracle[bj::ORACLE_STAGE2];
    s2.mono = mono_s2.p, s2.evals = s2_lde.p, s2.tree = s2_tree.p;
    if ((rc = intt_cols(s2_nat.p, mono_s2.p, nS2))) return rc;
    return commit(s2, s2_cap, MONOMIALS);
}

// Sharded quotient: this rank's Qe evaluations Tl [2][Qe] -> the coefficients of the whole quotient in T, on every rank.
// The first Qe points of this rank are s * H_Qe with s = x_{I0} = 7 * w_{Ln}^{bitrev(c0)}: the inverse transform
// with that shift gives R = T mod (x^Qe - a), a = s^Qe.  With T = sum_j x^(j Qe) T_j, R_i = sum_j a_i^j T_j: W residues
// (all-gathered: 2 Qe words from every rank, 2 q n in total) determine T by a W x W Vandermonde solve per coefficient
// (combine_residues_kernel) — no rank evaluates a point twice and the size-q n inverse transform is not replicated.
int Proving::exchange_residues(u64 *Tl) {
    const unsigned log_E = bj::log2_exact(Qe);
    auto rank_shift = [&](unsigned r) {
        return gl::mul(gl::GEN, gl::pow(gl::omega(log_n + S->log_L), gl::bitrev32(r * S->cl, S->log_L)));
    };
    int rc = bj_bitreverse_batch(ctx, Tl, Tl, log_E, 2, Qe);
    if (!rc) rc = bj_intt_batch(ctx, Tl, Tl, log_E, 2, Qe, rank_shift(sh.rank));
    if (rc) return rc;
    bj::TmpBuf all;
    if ((rc = all.take(ctx, bj::WS_RESIDUES))) return rc;
    if ((rc = bj::all_gather(ctx, sh, Tl, all.p, 2 * Qe))) return rc;
    u64 a[8];
    for (unsigned r = 0; r < sh.world; r++) a[r] = gl::pow(rank_shift(r), Qe);
    if (!bj::launch_combine_residues(all.p, sh.world, Qe, 2, a, T.p, st))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "sharded quotient: the residues' moduli are not distinct");
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

// ---------------- round 3: quotient (prover.rs:560-1495) ----------------
// Reads the witness, stage-2 and setup oracles, beta / gamma / lbeta / lgamma.  Draws alpha; adds T, the quotient oracle (its
// monomials: T's chunks in the monomial layout) and q_cap; the transcript absorbs q_cap.  Fails when the quotient is not a polynomial.
int Proving::round3_quotient() {
    const bool q_local = sh.world == 1;
    int rc = BJ_OK;
    u64 alpha[2];
    challenge2(alpha);
    const unsigned n_lookup_terms = L.n_lookup_terms;
    const unsigned n_gate_terms = S->gates.n_general_terms, n_spec_terms = S->gates.n_spec_terms;   // lookup | specialized | general | L1 | copy-permutation (prover.rs:599-625)
    const unsigned total_terms = n_lookup_terms + n_spec_terms + n_gate_terms + 1 + L.n_chunks;
    const std::vector<u64> alphas = e2_powers(alpha, total_terms);
    bj::TmpBuf d_alphas, T_local;
    if ((rc = d_alphas.take(ctx, bj::WS_ALPHAS, alphas.size()))) return rc;
    if ((rc = bj::h2d_async(ctx, d_alphas.p, alphas.data(), alphas.size() * 8))) return rc;
    if ((rc = T.take(ctx, bj::WS_T))) return rc;
    if (!q_local && (rc = T_local.take(ctx, bj::WS_T_LOCAL))) return rc;
    u64 *const Tl = q_local ? T.p : T_local.p;   // this rank's evaluations [2][Qe] (T itself when nothing has to be gathered)
    u64 *t0 = Tl, *t1 = Tl + Qe;
    const u64 *a_lookup = d_alphas.p, *a_spec = d_alphas.p + 2 * n_lookup_terms, *a_gates = a_spec + 2 * n_spec_terms,
              *a_l1 = a_gates + 2 * n_gate_terms;
    // Every term kernel on `points` points from local point `first` on, with the columns of the three oracles there given as
    // `wit`, `s2` and `setup`.  The accumulators are per point, so the whole range at once (every oracle is resident) and one coset
    // after the other (a lean one among them) write the same words.
    auto terms_on = [&](size_t first, size_t points, const bj::Cols wit, const bj::Cols s2, const bj::Cols setup) {
        auto sink = [&](const u64 *d_powers) { return bj::TermSink{d_powers, points, t0 + first, t1 + first}; };
        const bj::TermSink general = sink(a_gates), spec = sink(a_spec);
        bj::launch_circuit_gates(ctx, S, wit, setup.at(L.constant(0)), &general, &spec, st);
        if (has_lookup)
            bj::launch_quotient_lookup(bj::LookupArg{wit.at(L.lookup_var(0, 0)), setup.at(L.table(0)), S->tid_var ? nullptr : setup.at(L.table_id()).p,
                                                     wit.at(L.multiplicity()).p, S->lookup_reps, S->lookup_w, lbeta, lgamma},
                                       s2.at(L.lookup_a(0)).p, s2.at(L.lookup_b()).p, s2.stride, sink(a_lookup), st);
        // variables + sigmas + z and the partial products + 1/(x - 1), accumulators read and written
        const int pc = bj::probe_begin(ctx, "quotient_copy_perm", 8.0 * (2.0 * V + 2 * (1 + L.n_partials) + 1) * (double)points + 32.0 * (double)points);
        const u64 *h_alpha_l1 = alphas.data() + (a_l1 - d_alphas.p);   // the same power on the host: it goes into the kernel's arguments
        bj::launch_quotient_copy_perm(bj::CopyPermArg{wit, setup.at(L.sigma(0)), S->d_non_res, V, q, log_n, ctx->tw_fwd.p, beta, gamma, S->small_non_residues},
                                      s2, S->log_L, h_alpha_l1, sink(a_l1 + 2), I0 + first, S->d_inv_xm1 + first, st);
        bj::probe_end(ctx, pc);
    };
    bj::Oracle &wit = oracle[bj::ORACLE_WITNESS], &s2 = oracle[bj::ORACLE_STAGE2], &setup = oracle[bj::ORACLE_SETUP];
    if (wit.resident && s2.resident && setup.resident) {
        if (Qe) terms_on(0, Qe, wit.cols_at(0), s2.cols_at(0), setup.cols_at(0));
    } else {
        // An oracle that kept no evaluations has its columns extended from the monomials one coset at a time, and the terms of that
        // coset's n points are taken before the next one overwrites them; a resident one is read at that coset.  Highest coset
        // first, so that coset 0 is what stays in the buffers: round 4 evaluates the polynomials at z from it.  q == 0 cannot
        // happen (a power of two).  The quotient reads q cosets, the trees of rounds 1 and 2 covered fri_lde: neither bounds the other.
        if (!setup.resident) {
            if ((rc = setup_coset.take(ctx, bj::WS_SETUP_COSET))) return rc;
            setup.evals = setup_coset.p;
        }
        for (unsigned c = q; c-- > 0;) {
            for (const bj::Oracle *o : {&setup, &wit, &s2})
                if ((rc = rebuild(*o, c))) return rc;
            terms_on((size_t)c * n, n, wit.cols_at(c), s2.cols_at(c), setup.cols_at(c));
        }
    }
    BJ_CHECK_LAUNCH(ctx);
    // flatten (= bit-reversal of the evaluations), iNTT on their coset (prover.rs:1386-1422)
    if (q_local) {
        const unsigned log_Q = log_n + S->log_q;
        rc = bj_bitreverse_batch(ctx, T.p, T.p, log_Q, 2, Q);
        if (!rc) rc = bj_intt_batch(ctx, T.p, T.p, log_Q, 2, Q, gl::GEN);
    } else {
        rc = exchange_residues(Tl);
    }
    u64 top[2] = {1, 1};
    if (!rc) rc = bj_memcpy_d2h(ctx, &top[0], T.p + Q - 1, 8);
    if (!rc) rc = bj_memcpy_d2h(ctx, &top[1], T.p + 2 * Q - 1, 8);
    if (rc) return rc;
    if (top[0] != 0 || top[1] != 0)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove: constraint system is not satisfied (quotient is not a polynomial; prover.rs:1425-1438)");
    const u64 *Tm = T.p;   // the 2 q chunks of n coefficients each of the quotient, in the monomial layout of this trace length
    if (S->tiled) {   // the chunks come out of a transform of another size: one re-layout pass over 2 q n words
        bj::TmpBuf Tt;
        if ((rc = Tt.take(ctx, bj::WS_T_TILED))) return rc;
        bj::launch_tiled_permute(T.p, Tt.p, 2 * q, n, n, true, st);
        BJ_CHECK_LAUNCH(ctx);
        Tm = Tt.p;
    }
    if ((rc = q_lde.take(ctx, bj::WS_Q_LDE))) return rc;
    for (unsigned e = 0; e < 2 && !rc; e++)   // chunk j of c_e -> column 2j+e (prover.rs:1445-1467)
        rc = lde_cols(Tm + (size_t)e * Q, q_lde.p + (size_t)e * N, 2 * N, q, S->log_fri, sh.world > 1 ? S->c0 : 0, sh.world > 1 ? S->cl : S->fri_lde);
    if (rc) return rc;
    if ((rc = q_tree.take(ctx, bj::WS_Q_TREE))) return rc;
    bj::Oracle &quot = oracle[bj::ORACLE_QUOTIENT];
    quot.mono = Tm, quot.evals = q_lde.p, quot.tree = q_tree.p;
    return commit(quot, q_cap, EXTENDED);   // on the FRI domain, from the chunk layout: extended above
}

// Opened polynomials of the layout as sources on the evaluations of their oracles or on the monomials (oracle_value.h).  On the
// evaluations: from this rank's first coset on, which is all a lean oracle has (coset 0, left by round 3) — enough for round 4;
// DEEP reads a set there only if bj::can_stream says its oracles are on the FRI domain.
std::vector<Src> Proving::sources(const std::vector<bj::Opened> &polys, bool on_evals) const {
    std::vector<Src> ss;
    for (const bj::Opened &o : polys) ss.push_back(on_evals ? oracle[o.oracle].eval_src(o) : oracle[o.oracle].mono_src(o));
    return ss;
}

// The polynomials `ss` at the point `at`, by barycentric evaluation on this GPU's first coset (shift open_shift); w: 2 n words
// for the weights.  Sharded and many columns: every rank evaluates a slice and the values are all-gathered.
int Proving::evaluate_at(u64 *w, u64 open_shift, const std::vector<Src> &ss, const u64 *at, std::vector<u64> &vals) {
    int r = bj_barycentric_weights(ctx, log_n, open_shift, at, w, w + n);
    if (r) return r;
    const std::vector<const u64 *> ptrs = bj::open_columns(ss.data(), ss.size());
    std::vector<u64> raw(2 * ptrs.size());
    const size_t np = ptrs.size(), per = (np + sh.world - 1) / sh.world;
    if (sh.world > 1 && np >= 8 * (size_t)sh.world && 2 * per * sh.world <= bj::SmallBlock::GATHER_WORDS / 2) {
        // many columns: rank r evaluates the slice [r*per, (r+1)*per) on its own coset, the values are all-gathered
        // (the value of a polynomial does not depend on the coset it was interpolated from)
        const size_t lo = (size_t)sh.rank * per, hi = lo + per < np ? lo + per : np;
        std::vector<u64> mine(2 * per, 0);
        if (hi > lo) {
            r = bj_barycentric_eval_batch(ctx, ptrs.data() + lo, (unsigned)(hi - lo), log_n, w, w + n, mine.data());
            if (r) return r;
        }
        u64 *d_part = bj::gather_area(ctx), *d_all = bj::gather_half(ctx);
        if ((r = bj::h2d_async(ctx, d_part, mine.data(), 2 * per * 8))) return r;
        if ((r = bj::all_gather(ctx, sh, d_part, d_all, 2 * per))) return r;
        std::vector<u64> all(2 * per * sh.world);
        if ((r = bj_memcpy_d2h(ctx, all.data(), d_all, all.size() * 8))) return r;
        std::memcpy(raw.data(), all.data(), raw.size() * 8);
    } else {
        r = bj_barycentric_eval_batch(ctx, ptrs.data(), (unsigned)np, log_n, w, w + n, raw.data());
        if (r) return r;
    }
    vals.resize(2 * ss.size());
    bj::recombine_values(ss.data(), ss.size(), raw.data(), vals.data());
    return BJ_OK;
}

// ---------------- round 4: openings (prover.rs:1501-1802) ----------------
// Reads every oracle of rounds 1-3 on this rank's first coset.  Draws z; adds zo, vz, vzo, v0; the transcript absorbs the opened values.
int Proving::round4_openings() {
    int rc = BJ_OK;
    challenge2(z);
    bj::TmpBuf w;
    if ((rc = w.take(ctx, bj::WS_BARY_W))) return rc;
    const std::vector<bj::OpeningSet> sets = L.opening_sets(nullptr, nullptr, 0);   // everything at z, z(x) at z * omega, (lookups) the sums at 0
    // every rank evaluates from ITS first coset (shift 7*w^bitrev(c0)): the polynomials have degree < n, so the value
    // is the same field element whichever coset it is interpolated from — no exchange, identical transcripts
    const u64 open_shift = gl::mul(gl::GEN, gl::pow(gl::omega(log_n + S->log_L), gl::bitrev32(S->c0, S->log_L)));
    if ((rc = evaluate_at(w.p, open_shift, sources(sets[0].polys, true), z, vz))) return rc;
    tr.absorb(vz.data(), vz.size());
    {
        u64 om = gl::omega(log_n);
        zo[0] = gl::mul(gl::canon(z[0]), om);
        zo[1] = gl::mul(gl::canon(z[1]), om);
    }
    if ((rc = evaluate_at(w.p, open_shift, sources(sets[1].polys, true), zo, vzo))) return rc;
    tr.absorb(vzo.data(), vzo.size());
    if (has_lookup) {
        u64 zero2[2] = {0, 0};
        if ((rc = evaluate_at(w.p, open_shift, sources(sets[2].polys, true), zero2, v0))) return rc;
        tr.absorb(v0.data(), v0.size());
    }
    return BJ_OK;
}

// Round 5a's own state.  Every opening set goes the same way: the numerator sum_k ch_k f_k is a polynomial of degree < n, so it
// is combined on the MONOMIAL forms (n coefficients per column instead of the fri_lde_factor * n values of the FRI domain),
// extended by one two-column LDE and divided by (x - at) pointwise.  Exact arithmetic: the same values as combining on the LDE.
// The sets are prepared one after the other (a large one leaves its extended numerator in a buffer of its own) and divided
// by their (x - at) TOGETHER, bj::DEEP_MAX_SETS per launch: one inversion per lane for all of them, the destination written once.
struct DeepSets {
    std::vector<u64> chs;   // powers of the DEEP challenge, one per opened polynomial over all sets
    size_t choff = 0;       // challenges handed out so far
    bj::TmpBuf num_mono, num_slice;
    std::vector<bj::ColumnList> pending;   // the sets waiting for flush_deep, bj::DEEP_MAX_SETS per list = per launch
    bool written = false;   // deep holds the sets flushed so far

    void queue(const std::vector<Src> &ss, const u64 *ch, const u64 *vals, const u64 *at) {   // a source without a column: refused at the flush
        if (pending.empty() || pending.back().sets.size() == (size_t)bj::DEEP_MAX_SETS) pending.emplace_back();
        pending.back().add_set(ss.data(), ss.size(), ch, vals, at);
    }
};

// Divides the pending sets by their (x - at) into deep (accumulating once it has been written).
int Proving::flush_deep(DeepSets &D) {
    for (const bj::ColumnList &L : D.pending) {
        // DEEP, SURVEY §8d: 8 (#base columns) Ln + 16 Ln (the destination pair)
        const int pd = bj::probe_begin(ctx, "deep_accumulate_multi", 8.0 * (double)L.n_cols() * (double)N + (D.written ? 32.0 : 16.0) * (double)N);
        int r = bj::deep_accumulate_multi(ctx, L, log_n, S->log_fri, N, sh.world > 1 ? I0 : 0, deep.p, deep.p + N, D.written ? 1 : 0);
        bj::probe_end(ctx, pd);
        if (r) return r;
        D.written = true;
    }
    D.pending.clear();
    return BJ_OK;
}

// One opening set: the polynomials polys with the values vals at the point at.  Takes the next polys.size() challenges; queues
// the set for flush_deep: as it is, or (a large set, or one with a polynomial on no FRI domain: bj::can_stream) as its extended
// numerator, an arena buffer of 2 N words.
int Proving::deep_set(DeepSets &D, const std::vector<bj::Opened> &polys, const u64 *vals, const u64 *at) {
    const u64 *ch = D.chs.data() + 2 * D.choff;
    D.choff += polys.size();
    if (bj::base_columns(polys) < bj::WS_LARGE_SET && bj::can_stream(bj::oracle_mask(polys), bj::resident_mask(oracle))) {   // a handful of columns: streaming them over the FRI domain is cheaper than an extra LDE pass
        D.queue(sources(polys, true), ch, vals, at);
        return BJ_OK;
    }
    const std::vector<Src> ms = sources(polys, false);
    bj::TmpBuf num_lde;   // this set's extended numerator: alive until the sets are flushed
    if (int ra = num_lde.take(ctx, bj::WS_NUM_LDE)) return ra;
    int r;
    bj::ColumnList num;   // the numerator's columns and coefficients, and C = sum_k ch_k * v_k; unusable: combine_monomials refuses it
    if (sh.world > 1 && n % sh.world == 0 && n / sh.world >= 256) {
        // the monomials are replicated: every rank combines its slice of the coefficient range, one all-gather of the
        // two result columns rebuilds the numerator everywhere (the combination is the replicated part of DEEP)
        const size_t per = n / sh.world, off = (size_t)sh.rank * per;
        std::vector<Src> slice = ms;
        for (Src &m : slice) m = {m.c0 + off, m.c1 ? m.c1 + off : nullptr};
        num.add_set(slice.data(), slice.size(), ch, vals, at);
        r = bj::combine_monomials(ctx, num, per, D.num_slice.p, D.num_slice.p + per);
        if (!r) r = bj::all_gather_columns(ctx, sh, D.num_slice.p, D.num_mono.p, 2, per);
    } else {
        num.add_set(ms.data(), ms.size(), ch, vals, at);
        r = bj::combine_monomials(ctx, num, n, D.num_mono.p, D.num_mono.p + n);
    }
    if (r) return r;
    if (sh.world > 1)
        r = lde_cols(D.num_mono.p, num_lde.p, (size_t)S->cl << log_n, 2, S->log_L, S->c0, S->cl);
    else
        r = lde_cols(D.num_mono.p, num_lde.p, N, 2, S->log_fri, 0, S->fri_lde);
    if (r) return r;
    const u64 one[2] = {1, 0};   // one F_p^2 source (the extended numerator) with challenge 1 and "value" C
    D.queue({Src{num_lde.p, num_lde.p + N}}, one, num.sets[0].C, at);
    return BJ_OK;
}

// ---------------- round 5a: DEEP (prover.rs:1803-2067) ----------------
// Reads the opened columns and values of round 4, z / zo, the public inputs.  Draws the DEEP challenge; adds deep [2][N], the
// codeword FRI folds.
int Proving::round5a_deep() {
    int rc = BJ_OK;
    const std::vector<bj::OpeningSet> sets = L.opening_sets(S->pub_cols.data(), S->pub_rows.data(), S->pub_cols.size());
    u64 cch[2];
    challenge2(cch);
    size_t total_ch = 0;
    for (auto &set : sets) total_ch += set.polys.size();
    DeepSets D;
    D.chs = e2_powers(cch, total_ch);
    if ((rc = deep.take(ctx, bj::WS_DEEP))) return rc;
    if ((rc = D.num_mono.take(ctx, bj::WS_NUM_MONO))) return rc;
    if (sh.world > 1 && (rc = D.num_slice.take(ctx, bj::WS_NUM_SLICE))) return rc;
    const u64 zero2[2] = {0, 0};
    for (auto &set : sets) {   // in the order the challenges are handed out
        const u64 row[2] = {gl::pow(gl::omega(log_n), set.row), 0};
        std::vector<u64> pv;
        if (set.point == bj::OPEN_AT_ROW)
            for (unsigned v : set.value) pv.insert(pv.end(), {gl::canon(h_public_values[v]), 0});
        const u64 *const vals[4] = {vz.data(), vzo.data(), v0.data(), pv.data()}, *const at[4] = {z, zo, zero2, row};
        if ((rc = deep_set(D, set.polys, vals[set.point], at[set.point]))) return rc;
    }
    return flush_deep(D);
}

// ---------------- round 5b: FRI (prover.rs:2075-2105) ----------------
// Reads deep and the schedule (sched, sched_len, new_pow).  Adds the FRI object (its caps went through the transcript) and
// pow_challenge, absorbed as well.
int Proving::round5b_fri() {
    int rc = BJ_OK;
    bj_transcript trw;   // bj_fri_prove drives a bj_transcript; hand our state over and take it back
    trw.t = tr;
    rc = bj::fri_prove_sharded(ctx, sh, deep.p, deep.p + N, log_n, S->log_fri, sched, sched_len, S->cap_size, &trw, &fri);
    if (rc) return rc;
    tr = trw.t;
    // ---------------- proof of work (prover.rs:2107-2131; PoWRunner = Blake2s256, pow.rs:50-133, or Keccak256, pow.rs:139-230) ----------------
    if (new_pow) {
        u64 seed[5];   // 256 / CHAR_BITS = 4, "+1 if not a multiple of CHAR_BITS" -> 5 challenges = 40 seed bytes
        for (int i = 0; i < 5; i++) seed[i] = gl::canon(tr.challenge());
        bj::TmpBuf d_res;
        if ((rc = d_res.take(ctx, bj::WS_POW))) return rc;
        const u64 none = ~(u64)0, batch = (u64)1 << 24;
        u64 found = none;
        for (u64 base = 0; found == none; base += batch) {   // batches in order + minimum inside a batch = the smallest nonce,
            if ((rc = bj::h2d_async(ctx, d_res.p, &none, 8))) return rc;   // i.e. what the reference's serial search returns
            bj::launch_pow((int)S->pow_runner, seed, new_pow, base, batch, d_res.p, st);
            BJ_CHECK_LAUNCH(ctx);
            if ((rc = bj_memcpy_d2h(ctx, &found, d_res.p, 8))) return rc;
            if (base > ((u64)1 << 40)) return bj::fail(ctx, BJ_ERR_HIP, "bj_prove: proof of work did not terminate");
        }
        pow_challenge = found;
        const u64 lh[2] = {found & 0xFFFFFFFFULL, found >> 32};
        tr.absorb(lh, 2);
    }
    return BJ_OK;
}

// What round 6 hands to the serialiser
struct Queries {
    std::vector<u64> idxs;               // the queried leaves of the whole LDE domain
    unsigned depth = 0;                  // path length of the base oracles (witness, stage 2, quotient, setup)
    size_t block = 0;                    // words one rank gathered for the base oracles
    std::vector<u64> gathered;           // [rank][block]; query qi reads the block of rank idxs[qi] / N
    std::vector<std::vector<u64>> fri_leaves, fri_paths;   // per FRI oracle
    std::vector<unsigned> fri_depth;
};

// Round 6, the base oracles: leaves and Merkle paths of the witness, stage-2, quotient and setup trees.
// Reads qr.idxs, qr.depth, the four oracles; adds qr.block, qr.gathered.
int Proving::gather_base_queries(Queries &qr) {
    const unsigned W = sh.world, depth = qr.depth;
    // a leaf lives on rank index / N; every rank gathers at (index mod N) and the owner's answer is kept
    int rc = BJ_OK;
    bj::TmpBuf d_idx, d_g;
    size_t per_query = 0;
    for (const bj::Oracle &o : oracle) per_query += o.width + (size_t)depth * 4;
    const size_t G = qr.block = per_query * num_queries;
    if ((rc = d_idx.take(ctx, bj::WS_QUERY_IDX, num_queries))) return rc;
    if ((rc = d_g.take(ctx, bj::WS_QUERY_BLOCK, G))) return rc;
    {
        std::vector<u64> loc(num_queries);
        for (size_t i = 0; i < num_queries; i++) loc[i] = qr.idxs[i] % N;
        if ((rc = bj::h2d_async(ctx, d_idx.p, loc.data(), num_queries * 8))) return rc;
    }
    qr.gathered.resize(G * W);
    size_t off = 0;
    for (const bj::Oracle &o : oracle) {
        if (o.leaf_from_evals())
            bj::launch_gather_rows(o.evals, o.stride, o.width, d_idx.p, (unsigned)num_queries, d_g.p + off, st);
        else   // the leaf's words are the oracle's polynomials at the leaf's point (the monomials in the layout intt_cols writes); the paths come from the kept tree
            bj::launch_eval_monomials_at(o.mono, n, o.width, log_n, S->tiled, ctx->tw_fwd.p, I0, d_idx.p, (unsigned)num_queries, d_g.p + off, st);
        off += (size_t)o.width * num_queries;
        bj::launch_merkle_paths(o.tree, N, depth, d_idx.p, (unsigned)num_queries, d_g.p + off, st);
        off += (size_t)depth * 4 * num_queries;
    }
    BJ_CHECK_LAUNCH(ctx);
    const u64 *src = d_g.p;
    bj::TmpBuf all;
    if (W > 1) {
        if ((rc = all.take(ctx, bj::WS_QUERY_ALL, G * W))) return rc;
        if ((rc = bj::all_gather(ctx, sh, d_g.p, all.p, G))) return rc;
        src = all.p;
    }
    return bj_memcpy_d2h(ctx, qr.gathered.data(), src, qr.gathered.size() * 8);
}

// Round 6, the FRI openings, batched per oracle: leaf j = (index >> folds so far) >> k  (proof.rs:65-100, fri/mod.rs:829-895).
// Reads the FRI object and qr.idxs; adds qr.fri_leaves, qr.fri_paths, qr.fri_depth.
int Proving::gather_fri_queries(Queries &qr) {
    const size_t cap = S->cap_size;
    const unsigned W = sh.world;
    const std::vector<u64> &idxs = qr.idxs;
    int rc = BJ_OK;
    qr.fri_leaves.resize(sched_len), qr.fri_paths.resize(sched_len), qr.fri_depth.resize(sched_len);
    bj::TmpBuf d_li, d_fo;
    if ((rc = d_li.take(ctx, bj::WS_FRI_QUERY_IDX, num_queries))) return rc;
    size_t max_out = 0;
    for (size_t i = 0; i < sched_len; i++) {
        const bj_fri::Oracle &o = fri->oracles[i];
        qr.fri_depth[i] = bj::log2_exact(o.num_leaves / (cap / o.world));
        size_t need = ((size_t)2 << o.log_e) + (size_t)qr.fri_depth[i] * 4;
        if (need > max_out) max_out = need;
    }
    if ((rc = d_fo.take(ctx, bj::WS_FRI_QUERY_BLOCK, max_out * num_queries * (W + 1)))) return rc;
    std::vector<u64> li(num_queries), host_all;
    unsigned shift = 0;
    for (size_t i = 0; i < sched_len; i++) {
        const bj_fri::Oracle &o = fri->oracles[i];
        std::vector<u64> &leaves = qr.fri_leaves[i], &paths = qr.fri_paths[i];
        for (size_t qi = 0; qi < num_queries; qi++) li[qi] = ((idxs[qi] >> shift) >> o.log_e) % o.num_leaves;
        const unsigned shift0 = shift;
        shift += o.log_e;
        if ((rc = bj::h2d_async(ctx, d_li.p, li.data(), num_queries * 8))) return rc;
        const size_t E2 = (size_t)2 << o.log_e;
        bj::launch_gather_fri_leaves(o.d_c0, o.d_c1, o.log_e, d_li.p, (unsigned)num_queries, d_fo.p, st);
        bj::launch_merkle_paths(o.d_tree, o.num_leaves, qr.fri_depth[i], d_li.p, (unsigned)num_queries,
                                d_fo.p + E2 * num_queries, st);
        BJ_CHECK_LAUNCH(ctx);
        leaves.resize(E2 * num_queries);
        paths.resize((size_t)qr.fri_depth[i] * 4 * num_queries + 1);
        const size_t PD = (size_t)qr.fri_depth[i] * 4, blk = (E2 + PD) * num_queries;
        if (o.world > 1) {   // oracle 0 of a sharded proof: keep the owner's leaf and path
            u64 *d_all = d_fo.p + max_out * num_queries;
            if ((rc = bj::all_gather(ctx, sh, d_fo.p, d_all, blk))) return rc;
            host_all.resize(blk * W);
            if ((rc = bj_memcpy_d2h(ctx, host_all.data(), d_all, blk * W * 8))) return rc;
            for (size_t qi = 0; qi < num_queries; qi++) {
                const size_t owner = ((idxs[qi] >> shift0) >> o.log_e) / o.num_leaves;
                const u64 *b = host_all.data() + owner * blk;
                std::memcpy(leaves.data() + qi * E2, b + qi * E2, E2 * 8);
                std::memcpy(paths.data() + qi * PD, b + E2 * num_queries + qi * PD, PD * 8);
            }
            continue;
        }
        if ((rc = bj_memcpy_d2h(ctx, leaves.data(), d_fo.p, E2 * num_queries * 8))) return rc;
        if (PD && (rc = bj_memcpy_d2h(ctx, paths.data(), d_fo.p + E2 * num_queries, PD * num_queries * 8))) return rc;
    }
    return BJ_OK;
}

// ---------------- round 6: queries (prover.rs:2161-2266) ----------------
// Reads the transcript (query indices), every oracle and tree of the proof.  Adds qr.
int Proving::round6_queries(Queries &qr) {
    bj::host::BoolsBuffer bools;
    bools.max_needed = log_n + S->log_fri;
    qr.idxs.resize(num_queries);
    for (size_t i = 0; i < num_queries; i++) qr.idxs[i] = bools.query_index(tr, log_n, S->log_fri);
    qr.depth = bj::log2_exact(N / capl);
    if (int rc = gather_base_queries(qr)) return rc;
    return gather_fri_queries(qr);
}

// ---------------- serialise ----------------
// Reads the caps, the opened values, the FRI object and the query answers; fills proof->data (word order: proof_layout.h; parsed by proof_format.py).
int Proving::serialise(const Queries &qr) {
    const size_t cap = S->cap_size, n_pub = S->pub_cols.size();
    const bj::SerialLayout SL = bj::serial_layout(L, sched, sched_len, final_degree, num_queries, n_pub);
    if (!SL.ok) return bj::fail(ctx, BJ_ERR_HIP, "bj_prove: internal error: the proof's own schedule has no serialised layout");
    const size_t depth4 = (size_t)SL.depth * 4;
    std::vector<u64> &D = proof->data;
    D.assign(SL.total, 0);
    auto put = [&](size_t at, const u64 *p, size_t k) { std::copy(p, p + k, D.begin() + at); };
    bj::ProofHeader header;
    header.fill(L, n_pub, sched_len, final_degree, num_queries, SL.depth, S->pow_bits, pow_challenge);
    put(SL.header, header.w, bj::ProofHeader::WORDS);
    for (size_t i = 0; i < sched_len; i++) D[SL.schedule + i] = sched[i];
    for (size_t i = 0; i < n_pub; i++) D[SL.public_inputs + i] = gl::canon(h_public_values[i]);
    put(SL.witness_cap, wit_cap.data(), wit_cap.size());
    put(SL.stage2_cap, s2_cap.data(), s2_cap.size());
    put(SL.quotient_cap, q_cap.data(), q_cap.size());
    put(SL.values_at_z, vz.data(), vz.size());
    put(SL.values_at_z_omega, vzo.data(), vzo.size());
    put(SL.values_at_0, v0.data(), v0.size());
    {
        std::vector<u64> c(4 * cap);
        for (size_t i = 0; i < sched_len; i++) {
            bj_fri_cap(fri, i, c.data());
            put(SL.fri_caps + i * c.size(), c.data(), c.size());
        }
        std::vector<u64> f0(final_degree), f1(final_degree);
        bj_fri_final_monomials(fri, f0.data(), f1.data());
        put(SL.final_c0, f0.data(), final_degree);
        put(SL.final_c1, f1.data(), final_degree);
    }
    for (size_t qi = 0; qi < num_queries; qi++) {
        const size_t at = SL.queries + qi * SL.query_words;
        D[at] = qr.idxs[qi];
        size_t off = (qr.idxs[qi] / N) * qr.block;   // the block of the rank that owns the leaf: per oracle [leaves][paths]
        for (int o = 0; o < 4; o++) {
            put(at + SL.leaf_off[o], qr.gathered.data() + off + qi * L.widths[o], L.widths[o]);
            off += (size_t)L.widths[o] * num_queries;
            put(at + SL.path_off[o], qr.gathered.data() + off + qi * depth4, depth4);
            off += depth4 * num_queries;
        }
        for (size_t i = 0; i < sched_len; i++) {
            const size_t E2 = (size_t)2 << sched[i];
            put(at + SL.fri_leaf_off[i], qr.fri_leaves[i].data() + qi * E2, E2);
            put(at + SL.fri_path_off[i], qr.fri_paths[i].data() + qi * (size_t)SL.fri_depth[i] * 4, (size_t)SL.fri_depth[i] * 4);
        }
    }
    return BJ_OK;
}

// The proof has drained (its bytes are on the host): the collectives' event pairs and the kernel probes can be read.
// Adds the communication, kernel and workspace statistics of the proof; the context learns the workspace it took.
void Proving::read_back_stats() {
    float ms = ctx->comm_host_ms;
    const unsigned n_stream = ctx->comm_n & 0xFFFFu;
    for (unsigned i = 0; i < n_stream; i++) {
        float e = 0;
        if (hipEventElapsedTime(&e, ctx->comm_ev[i][0], ctx->comm_ev[i][1]) == hipSuccess) ms += e;
    }
    proof->comm_ms = ms;
    proof->comm_calls = n_stream + (ctx->comm_n >> 16);
    proof->comm_bytes = ctx->comm_bytes;
    for (unsigned i = 0; i < ctx->probe_n; i++) {
        float e = 0;
        if (!ctx->probes[i].closed) continue;   // its closing record failed: the event still belongs to an earlier proof
        if (hipEventElapsedTime(&e, ctx->probes[i].ev[0], ctx->probes[i].ev[1]) != hipSuccess) continue;
        proof->kernel_stats[proof->n_kernel_stats++] = {ctx->probes[i].name, e, ctx->probes[i].bytes};
    }
    proof->ws_high_water = ctx->bump.high_water * 8;
    proof->ws_overflow_slabs = ctx->bump.slabs.size();
    // the context learns from a proof that outgrew its reservation; one that stayed inside it (every proof whose plan holds: the
    // reservation of a single-GPU proof IS its high-water mark) leaves the arena as it is, so the next proof re-allocates nothing
    if (proof->ws_overflow_slabs && ctx->bump.high_water + ((size_t)1 << 17) > ctx->arena_learned)
        ctx->arena_learned = ctx->bump.high_water + ((size_t)1 << 17);
}

// Scope guards of a proof.  prove_impl declares them in this order, so they end in the reverse one: the FRI object first,
// then the copy stream is drained, the tree hasher and the in_proof flag return, and a proof that did not finish is deleted.
struct ProofGuard {
    bj_proof *&p;
    bool ok = false;
    ~ProofGuard() {
        if (!ok) {
            delete p;
            p = nullptr;
        }
    }
};
struct InProof {   // temporaries of the ABI calls of the rounds come out of the arena while this is alive
    bj_ctx *c;
    InProof(bj_ctx *x, const bj::WorkspacePlan *plan) : c(x) {
        c->in_proof = true;
        c->ws_plan = plan;
        c->ws_next = 0;
        c->comm_n = 0;
        c->comm_bytes = 0;
        c->comm_host_ms = 0;
        c->probe_n = 0;
    }
    ~InProof() {
        c->in_proof = false;
        c->ws_plan = nullptr;
    }
};
struct CopyDrain {   // bj_prove, bj_prove_values: whatever way the proof ends, no queued copy may still read the caller's witness afterwards
    bj_ctx *c;
    bool active;
    ~CopyDrain() {
        if (active && c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    }
};
struct FriGuard {
    bj_fri *&f;   // nullptr until round 5b
    ~FriGuard() { bj_fri_destroy(f); }
};

int prove_impl(bj_ctx *ctx, const bj_setup *S, const uint64_t *d_variables, const uint64_t *d_multiplicities,
               const uint64_t *h_public_values, bj_proof **out, const HostWitness *hw, bool count, const ValuesWitness *vw = nullptr) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_dev: null out pointer");
    *out = nullptr;
    if (!S || !d_variables) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_dev: null argument");
    if (!S->pub_cols.empty() && !h_public_values) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_dev: public input values required");
    int rc = BJ_OK;
    Proving P(ctx, S, d_variables, d_multiplicities, h_public_values, hw, vw, count);
    P.proof = new bj_proof();
    ProofGuard guard{P.proof};
    if ((rc = P.reserve_workspace())) return rc;
    InProof in_proof(ctx, &P.plan);
    bj::HasherGuard hasher_guard{ctx, ctx->hasher};
    CopyDrain copy_drain{ctx, hw != nullptr || vw != nullptr};
    ctx->hasher = (int)S->hasher;
    if ((rc = P.check_public_inputs())) return rc;
    StageTimer timer(P.st);
    FriGuard fri_guard{P.fri};
    float *stage_ms = P.proof->stage_ms;
    if ((rc = P.open_transcript())) return rc;
    if ((rc = P.round1_witness())) return rc;
    stage_ms[0] = timer.lap();
    if ((rc = P.round2_stage2())) return rc;
    stage_ms[1] = timer.lap();
    if ((rc = P.round3_quotient())) return rc;
    stage_ms[2] = timer.lap();
    if ((rc = P.round4_openings())) return rc;
    stage_ms[3] = timer.lap();
    if ((rc = P.round5a_deep())) return rc;
    stage_ms[4] = timer.lap();
    if ((rc = P.round5b_fri())) return rc;
    stage_ms[5] = timer.lap();
    Queries qr;
    if ((rc = P.round6_queries(qr))) return rc;
    if ((rc = P.serialise(qr))) return rc;
    if ((rc = bj::workspace_all_taken(ctx))) return rc;
    stage_ms[6] = timer.lap();
    P.read_back_stats();
    guard.ok = true;
    *out = P.proof;
    return BJ_OK;
}

}  // namespace

extern "C" {

static int stage_witness(bj_ctx *ctx, const bj_setup *S) {
    const size_t n = (size_t)1 << S->log_n, need = (size_t)(S->layout.multiplicity() + 1) * n;   // the multiplicity column behind the others
    return bj::stage_witness_elems(ctx, need);
}

int bj_prove_dev(bj_ctx *ctx, const bj_setup *S, const uint64_t *d_variables, const uint64_t *d_multiplicities,
                 const uint64_t *h_public_values, bj_proof **out) {
    return prove_impl(ctx, S, d_variables, d_multiplicities, h_public_values, out, nullptr, d_multiplicities == nullptr);   // NULL: counted
}

int bj_prove(bj_ctx *ctx, const bj_setup *S, const uint64_t *h_variables, const uint64_t *h_multiplicities,
             const uint64_t *h_public_values, bj_proof **out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!S || !h_variables || !out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove: null argument");
    if (int rc = stage_witness(ctx, S)) return rc;
    const size_t n = (size_t)1 << S->log_n;
    const unsigned group = bj::env().prove_h2d_group;
    const HostWitness hw{h_variables, h_multiplicities, group, false};
    // the copies are queued inside the proof (after the workspace is reserved); a previous proof on this context has drained
    return prove_impl(ctx, S, ctx->wit_stage.p, ctx->wit_stage.p + (size_t)S->layout.multiplicity() * n, h_public_values, out, &hw, h_multiplicities == nullptr);
}

int bj_prove_values(bj_ctx *ctx, const bj_setup *S, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                    size_t n_multiplicities, bj_proof **out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove_values: null out pointer");
    *out = nullptr;
    if (int rc = bj::values_check(ctx, "bj_prove_values", S, h_values, n_values, h_multiplicities, n_multiplicities)) return rc;
    return bj::prove_values_staged(ctx, S, h_values, n_values, h_multiplicities, n_multiplicities, out, false);
}

}  // extern "C"

namespace bj {
// What bj_prove_values and bj_prove_values_async refuse before anything is queued; `who` starts the messages.
int values_check(bj_ctx *ctx, const char *who, const bj_setup *S, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                 size_t n_multiplicities) {
    if (!S) return fail(ctx, BJ_ERR_INVALID_ARG, "%s: null argument", who);
    if (S->sh.world != 1)
        return fail(ctx, BJ_ERR_UNSUPPORTED, "%s: single-device setups only (a sharded setup holds no placement)", who);
    if (!S->d_placement)
        return fail(ctx, BJ_ERR_INVALID_ARG, "%s: the setup holds no variable placement (make it with bj_setup_create_from_placement)", who);
    if (S->Wc && !S->d_wit_placement)
        return fail(ctx, BJ_ERR_INVALID_ARG, "%s: the setup has %u non-copiable witness columns and no witness placement "
                                             "(bj_setup_set_witness_placement)", who, S->Wc);
    if (n_values && !h_values) return fail(ctx, BJ_ERR_INVALID_ARG, "%s: null h_values with n_values %zu", who, n_values);
    if (n_values > PLACEMENT_NONE) return fail(ctx, BJ_ERR_UNSUPPORTED, "%s: n_values %zu above 2^32 - 1 (the placement is u32)", who, n_values);
    const size_t n = (size_t)1 << S->log_n;
    if (n_multiplicities > n) return fail(ctx, BJ_ERR_INVALID_ARG, "%s: %zu multiplicities for %zu rows", who, n_multiplicities, n);
    if (n_multiplicities && !h_multiplicities) return fail(ctx, BJ_ERR_INVALID_ARG, "%s: null h_multiplicities with n_multiplicities %zu", who, n_multiplicities);
    if (S->pub_place.size() != S->pub_cols.size()) return fail(ctx, BJ_ERR_HIP, "%s: internal error: no placement entries for the public inputs", who);
    for (uint32_t entry : S->pub_place)
        if (entry != PLACEMENT_NONE && entry >= n_values) return fail(ctx, BJ_ERR_INVALID_ARG, "%s: a cell names a variable beyond all_values", who);
    return BJ_OK;
}

// words of the witness staging of a proof from values: cells and multiplicity column, all_values, the u32 counters (lane_extras)
static size_t values_staging_words(const bj_setup *S, size_t n_values) {
    const size_t n = (size_t)1 << S->log_n;
    return (size_t)(S->layout.multiplicity() + 1) * n + values_staging_bytes(n, n_values ? n_values : 1) / 8;
}

// The proof of bj_prove_values on a context whose checks have passed (values_check): by the calling thread, or by a lane of
// bj_prove_values_async (no_absorb: its sibling is proving, the leaves are hashed once at the end).
int prove_values_staged(bj_ctx *ctx, const bj_setup *S, const uint64_t *h_values, size_t n_values, const uint32_t *h_multiplicities,
                        size_t n_multiplicities, bj_proof **out, bool no_absorb) {
    if (int rc = bind(ctx)) return rc;
    if (int rc = stage_witness_elems(ctx, values_staging_words(S, n_values))) return rc;
    const size_t n = (size_t)1 << S->log_n, vw_cols = S->layout.multiplicity();
    u64 *stage = ctx->wit_stage.p, *d_values = stage + (vw_cols + 1) * n;
    const ValuesWitness vw{h_values, n_values, h_multiplicities, n_multiplicities, d_values, reinterpret_cast<uint32_t *>(d_values + (n_values ? n_values : 1)),
                           env().prove_h2d_group, no_absorb};
    // a public input is the cell at its location: all_values at the placement entry the setup kept, 0 on a placeholder.  h_values
    // may be a view into a dump (bj_prove_from_dumps) and unaligned: read with memcpy
    std::vector<u64> pub(S->pub_place.size() ? S->pub_place.size() : 1, 0);
    for (size_t i = 0; i < S->pub_place.size(); i++)
        if (S->pub_place[i] != PLACEMENT_NONE) std::memcpy(&pub[i], reinterpret_cast<const unsigned char *>(h_values) + (size_t)S->pub_place[i] * 8, 8);
    return prove_impl(ctx, S, stage, stage + vw_cols * n, pub.data(), out, nullptr, S->layout.has_lookup && h_multiplicities == nullptr, &vw);
}

// What a lane of bj_prove_async wants for a proof of S from a host witness (async_admission.h), its witness and stage-2 oracles
// resident and lean.  The lane may take the proof as bj_prove or witness first (prove_host_copy_first): the plan of bj_prove where
// it absorbs the column groups holds every buffer of the others and the capacity words, so that one is reserved.  Where
// BJ_PROOF_LEAN makes every proof lean, both are the lean footprint.  values: the proof is bj_prove_values_async's with that many
// values (the staging holds them and the counters as well; an empty all_values counts as one word).
int async_footprints(bj_ctx *ctx, const bj_setup *S, LaneBytes *resident, LaneBytes *lean, bool values, size_t n_values) {
    uint32_t sched[32], new_pow = 0;
    size_t sched_len = 0, num_queries = 0, final_degree = 0;
    if (int rc = bj_fri_schedule(S->security, S->cap_size, S->pow_bits, S->log_fri, S->log_n, &new_pow, &num_queries, sched, &sched_len, &final_degree))
        return fail(ctx, rc, "bj_prove_async: compute_fri_schedule failed");
    const bool absorbs = (S->hasher == BJ_HASHER_POSEIDON2 || S->hasher == BJ_HASHER_POSEIDON) && !env().prove_no_absorb;
    WorkspaceShape shape = shape_of(S, false, absorbs ? WS_HOST_ABSORBING : WS_HOST_NOT_ABSORBING, false, new_pow, sched, sched_len, num_queries);
    if (values) shape.n_values = n_values ? n_values : 1;
    *lean = lane_footprint(shape, true);
    *resident = env().proof_lean ? *lean : lane_footprint(shape, false);
    return BJ_OK;
}

// bj_prove for a lane of bj_prove_async whose sibling is busy: the whole witness crosses PCIe first (one copy on the proof's
// stream, while the other lane's proof has the CUs), then the proof runs as on a resident witness — one leaf kernel instead of
// the group-wise absorption that bj_prove uses to hide the transfer behind its own hashing.  Same bytes either way.
int prove_host_copy_first(bj_ctx *ctx, const bj_setup *S, const uint64_t *h_variables, const uint64_t *h_multiplicities,
                          const uint64_t *h_public_values, bj_proof **out, int mode) {
    if (int rc = bind(ctx)) return rc;
    if (!S || !h_variables || !out) return fail(ctx, BJ_ERR_INVALID_ARG, "bj_prove: null argument");
    if (int rc = stage_witness(ctx, S)) return rc;
    const size_t n = (size_t)1 << S->log_n, vw = (size_t)S->layout.multiplicity() * n;
    if (mode == 2) {   // transfer and transform in groups as bj_prove does, but ONE leaf kernel at the end: the sibling lane's kernels
                       // cover the transfer, so nothing is gained by absorbing group by group (extra launches, capacity round trips)
        const HostWitness hw{h_variables, h_multiplicities, env().prove_h2d_group, true};
        return prove_impl(ctx, S, ctx->wit_stage.p, ctx->wit_stage.p + vw, h_public_values, out, &hw, h_multiplicities == nullptr);
    }
    BJ_HIP(ctx, hipMemcpyAsync(ctx->wit_stage.p, h_variables, vw * 8, hipMemcpyHostToDevice, ctx->stream));
    if (S->lookup_reps && h_multiplicities) BJ_HIP(ctx, hipMemcpyAsync(ctx->wit_stage.p + vw, h_multiplicities, n * 8, hipMemcpyHostToDevice, ctx->stream));
    const int rc = prove_impl(ctx, S, ctx->wit_stage.p, ctx->wit_stage.p + vw, h_public_values, out, nullptr, h_multiplicities == nullptr);
    (void)hipStreamSynchronize(ctx->stream);   // no queued copy may read the caller's witness after this returns
    return rc;
}
}  // namespace bj
