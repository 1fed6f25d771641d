// bj_check_satisfied: where a witness fails its circuit (the role of CSReferenceAssembly::check_if_satisfied,
// src/cs/implementations/satisfiability_test.rs:15-353, extended to the lookup argument), on the replicated natural-order
// columns of a setup.  Three parts:
//   gates    phase 1: every evaluator of the circuit once over the n trace rows (launch_circuit_gates, the block the quotient stage
//            runs on the LDE) with fixed pseudo-random F_p^2 weights, then one reduction for the first non-zero row and their
//            number; phase 2, only on a failure: that one row, replicated over a block of points, term by term with unit weights.
//   lookups  the index over the table rows of lookup_index.h (classes of equal rows, representative = smallest row), one probe
//            per looked-up tuple, then expected (sum of the class's multiplicities) against counted per class.
//   report   first failure in the order of include/boojum_hip.h.
// All scratch is the context's (ensure_scratch); nothing here allocates, and no input is written.
#include "check_shared.h"
#include "ctx.h"
#include "lookup_index.h"
#include "setup.h"

#include <cstring>
#include <vector>

using gl::u64;
using namespace bj::lookup;   // LookupShape, find_class, lookup_build_kernel, block_min_count, the slot conventions
using namespace bj::check;    // CHECK_BLOCK, the weights, lookup_expected_kernel, expected_value (check_shared.h)

namespace {

// counters the kernels reduce into: [2k] smallest key, [2k + 1] number, k = bj_unsat_kind - 1
struct Counters {
    u64 v[8];
};

// rows whose weighted sum of terms is not zero
__global__ void __launch_bounds__(CHECK_BLOCK) nonzero_rows_kernel(const u64 *t0, const u64 *t1, size_t n, u64 *out_min, u64 *out_cnt) {
    const size_t i = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) bad = (gl::canon(t0[i]) | gl::canon(t1[i])) != 0;
    block_min_count(bad, (u64)i, out_min, out_cnt);
}

// one trace row of `cols` columns: replicated over CHECK_BLOCK points (column c at out + c * CHECK_BLOCK) and once into flat[c]
__global__ void __launch_bounds__(CHECK_BLOCK) replicate_row_kernel(const u64 *src, size_t stride, unsigned cols, size_t row, u64 *out, u64 *flat) {
    const unsigned c = blockIdx.x;
    if (c >= cols) return;
    const u64 v = gl::canon(src[(size_t)c * stride + row]);
    out[(size_t)c * CHECK_BLOCK + threadIdx.x] = v;
    if (threadIdx.x == 0) flat[c] = v;
}

// one thread per (sub-argument, row): count[class] += 1, or a miss keyed row * reps + sub-argument
__global__ void __launch_bounds__(CHECK_BLOCK) lookup_probe_kernel(LookupShape L, const uint32_t *slots, unsigned long long *count, u64 *miss_min,
                                                                  u64 *miss_cnt) {
    const size_t i = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    const bool live = i < L.n * L.reps;
    uint32_t cls = SLOT_EMPTY;
    u64 key = NONE64;
    if (live) {
        const size_t sub = i / L.n, row = i - sub * L.n;
        u64 t[MAX_TUPLE];
        load_looked_up(L, sub, row, t);
        cls = find_class(L, slots, t);
        key = (u64)row * L.reps + sub;
    }
    const bool hit = live && cls != SLOT_EMPTY;
    // the lanes that hit the class of the first hitting lane share one atomic (unused sub-arguments all look the same tuple up)
    const u64 hits = __ballot(hit);
    if (hits) {
        const int leader = __ffsll((long long)hits) - 1;
        const uint32_t c0 = __shfl(cls, leader);
        const u64 same = __ballot(hit && cls == c0);
        if ((int)lane_id() == leader) atomicAdd(count + c0, (unsigned long long)__popcll(same));
        if (hit && cls != c0) atomicAdd(count + cls, 1ull);
    }
    block_min_count(live && !hit, key, miss_min, miss_cnt);
}

// one thread per table row; a representative compares its class's sum with its count (an integer below p)
__global__ void __launch_bounds__(CHECK_BLOCK) lookup_compare_kernel(size_t n, const uint32_t *class_of, const unsigned long long *count,
                                                                    const unsigned long long *lo, const uint32_t *hi, u64 *bad_min, u64 *bad_cnt) {
    const size_t r = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    bool bad = false;
    if (r < n && class_of[r] == (uint32_t)r) bad = expected_value(lo[r], hi[r]) != (u64)count[r];
    block_min_count(bad, (u64)r, bad_min, bad_cnt);
}

int check_impl(bj_ctx *ctx, const bj_setup *S, const u64 *d_variables, const u64 *d_multiplicities, bj_unsat_report *out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!S || !d_variables || !out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_satisfied: null argument");
    if (S->device != ctx->device) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_satisfied: the setup lives on device %d, the context on %d", S->device, ctx->device);
    const bool has_lookup = S->lookup_reps > 0;
    if (has_lookup && !d_multiplicities) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_satisfied: multiplicities required");
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_satisfied: a proof is running on this context");
    if (S->log_n > 30) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_check_satisfied: traces above 2^30 rows (table rows are kept as 32-bit numbers)");
    if (has_lookup && S->lookup_w + 1 > MAX_TUPLE) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_check_satisfied: lookup width %u above %u", S->lookup_w, MAX_TUPLE - 1);
    std::memset(out, 0, sizeof(*out));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << S->log_n, B = CHECK_BLOCK;
    const bj::ProofLayout &PL = S->layout;
    const unsigned VW = S->V + S->Wc, nC = S->nC;
    const u64 *d_consts = S->d_nat + (size_t)PL.constant(0) * n;

    // terms in evaluator order: (gate, repetition, term), general-purpose gates first
    const unsigned n_gate_terms = S->gates.n_general_terms, n_spec_terms = S->gates.n_spec_terms, n_terms = n_gate_terms + n_spec_terms;
    const unsigned M = (n_gate_terms > n_spec_terms ? n_gate_terms : n_spec_terms) + 1;

    // scratch layout (words)
    size_t off = 0;
    auto take = [&off](size_t words) {
        const size_t at = off;
        off += (words + 1) & ~(size_t)1;   // 16-byte alignment for every block
        return at;
    };
    const size_t o_t = take(2 * n), o_ctr = take(8), o_alpha = take(2 * (size_t)n_terms + 2), o_unit = take(2 * (2 * (size_t)M + 1));
    const size_t o_row_v = take((size_t)VW * B), o_row_c = take((size_t)nC * B), o_flat = take((size_t)VW + nC), o_tb = take((size_t)M * 2 * B);
    const size_t o_slots = has_lookup ? take(n) : 0, o_count = has_lookup ? take(n) : 0, o_lo = has_lookup ? take(n) : 0;
    const size_t o_hi = has_lookup ? take(n / 2 + 1) : 0, o_cls = has_lookup ? take(n / 2 + 1) : 0;
    if (int rc = bj::ensure_scratch(ctx, off)) return rc;
    u64 *W = ctx->d_scratch.p;
    u64 *t0 = W + o_t, *t1 = t0 + n, *ctr = W + o_ctr, *d_alpha = W + o_alpha, *d_unit = W + o_unit;

    {
        Counters c;
        for (int k = 0; k < 4; k++) {
            c.v[2 * k] = NONE64;
            c.v[2 * k + 1] = 0;
        }
        if (int rc = bj::h2d_async(ctx, ctr, c.v, sizeof(c.v))) return rc;
        std::vector<u64> alphas(2 * (size_t)n_terms + 2, 0);
        u64 state = ALPHA_SEED;
        for (size_t i = 0; i < 2 * (size_t)n_terms; i++) alphas[i] = splitmix64(state) % gl::P;
        if (int rc = bj::h2d_async(ctx, d_alpha, alphas.data(), alphas.size() * 8)) return rc;
    }

    // ---- gates, phase 1 ----
    const bj::Cols trace_vars{d_variables, n}, trace_consts{d_consts, n};
    const bj::TermSink general{d_alpha, n, t0, t1}, spec{d_alpha + 2 * (size_t)n_gate_terms, n, t0, t1};
    if (n_gate_terms) {
        bj::launch_circuit_gates(ctx, S, trace_vars, trace_consts, &general, nullptr, st);
        hipLaunchKernelGGL(nonzero_rows_kernel, dim3(blocks_for(n)), dim3(CHECK_BLOCK), 0, st, t0, t1, n, ctr + 0, ctr + 1);
    }
    if (n_spec_terms) {
        BJ_HIP(ctx, hipMemsetAsync(t0, 0, 2 * n * 8, st));
        bj::launch_circuit_gates(ctx, S, trace_vars, trace_consts, nullptr, &spec, st);
        hipLaunchKernelGGL(nonzero_rows_kernel, dim3(blocks_for(n)), dim3(CHECK_BLOCK), 0, st, t0, t1, n, ctr + 2, ctr + 3);
    }
    BJ_CHECK_LAUNCH(ctx);

    // ---- lookups ----
    unsigned long long *d_count = nullptr, *d_lo = nullptr;
    uint32_t *d_hi = nullptr;
    if (has_lookup) {
        uint32_t *slots = (uint32_t *)(W + o_slots), *class_of = (uint32_t *)(W + o_cls);
        d_count = (unsigned long long *)(W + o_count);
        d_lo = (unsigned long long *)(W + o_lo);
        d_hi = (uint32_t *)(W + o_hi);
        BJ_HIP(ctx, hipMemsetAsync(slots, 0xFF, 2 * n * sizeof(uint32_t), st));
        BJ_HIP(ctx, hipMemsetAsync(d_count, 0, n * 8, st));
        BJ_HIP(ctx, hipMemsetAsync(d_lo, 0, n * 8, st));
        BJ_HIP(ctx, hipMemsetAsync(d_hi, 0, n * 4, st));
        LookupShape L;
        L.tables = S->d_nat + (size_t)PL.table(0) * n;
        L.lvars = d_variables + (size_t)PL.lookup_var(0, 0) * n;
        L.table_id = S->tid_var ? nullptr : S->d_nat + (size_t)PL.table_id() * n;
        L.n = L.tstride = L.vstride = n;
        L.w = S->lookup_w;
        L.reps = S->lookup_reps;
        L.cps = S->lookup_cps;
        L.mask = (uint32_t)(2 * n - 1);
        hipLaunchKernelGGL(lookup_build_kernel, dim3(blocks_for(n)), dim3(CHECK_BLOCK), 0, st, L, slots);
        hipLaunchKernelGGL(lookup_probe_kernel, dim3(blocks_for(n * L.reps)), dim3(CHECK_BLOCK), 0, st, L, (const uint32_t *)slots, d_count, ctr + 4, ctr + 5);
        hipLaunchKernelGGL(lookup_expected_kernel, dim3(blocks_for(n)), dim3(CHECK_BLOCK), 0, st, L, (const uint32_t *)slots, d_multiplicities, class_of,
                           d_lo, d_hi);
        hipLaunchKernelGGL(lookup_compare_kernel, dim3(blocks_for(n)), dim3(CHECK_BLOCK), 0, st, n, (const uint32_t *)class_of,
                           (const unsigned long long *)d_count, (const unsigned long long *)d_lo, (const uint32_t *)d_hi, ctr + 6, ctr + 7);
        BJ_CHECK_LAUNCH(ctx);
    }
    Counters c;
    if (int rc = bj_memcpy_d2h(ctx, c.v, ctr, sizeof(c.v))) return rc;   // synchronises
    for (int k = 0; k < 4; k++) out->failures[k + 1] = c.v[2 * k + 1];
    int kind = BJ_SAT;
    for (int k = 3; k >= 0; k--)
        if (c.v[2 * k + 1]) kind = k + 1;
    out->kind = (uint32_t)kind;
    if (kind == BJ_SAT) return BJ_OK;

    if (kind == BJ_UNSAT_LOOKUP) {
        out->row = c.v[4] / S->lookup_reps;
        out->gate = (uint32_t)(c.v[4] % S->lookup_reps);
        return BJ_OK;
    }
    if (kind == BJ_UNSAT_MULTIPLICITY) {
        const u64 r = c.v[6];
        u64 cnt = 0, lo = 0;
        uint32_t hi = 0;
        int rc = bj_memcpy_d2h(ctx, &cnt, d_count + r, 8);
        if (!rc) rc = bj_memcpy_d2h(ctx, &lo, d_lo + r, 8);
        if (!rc) rc = bj_memcpy_d2h(ctx, &hi, d_hi + r, 4);
        if (rc) return rc;
        out->row = r;
        out->value = cnt;
        out->expected = expected_value(lo, hi);
        return BJ_OK;
    }

    // ---- gates, phase 2: the failing row alone, one term at a time with unit weights ----
    const u64 row = kind == BJ_UNSAT_GATE ? c.v[0] : c.v[2];
    u64 *row_v = W + o_row_v, *row_c = W + o_row_c, *flat = W + o_flat, *tb = W + o_tb;
    std::vector<u64> unit(2 * (2 * (size_t)M + 1), 0);
    unit[2 * (size_t)M] = 1;   // seen from d_unit + 2 * (M - k), term k has weight (1, 0) and every other term (0, 0)
    if (int rc = bj::h2d_async(ctx, d_unit, unit.data(), unit.size() * 8)) return rc;
    hipLaunchKernelGGL(replicate_row_kernel, dim3(VW), dim3(CHECK_BLOCK), 0, st, d_variables, n, VW, (size_t)row, row_v, flat);
    if (nC) hipLaunchKernelGGL(replicate_row_kernel, dim3(nC), dim3(CHECK_BLOCK), 0, st, d_consts, n, nC, (size_t)row, row_c, flat + VW);
    BJ_CHECK_LAUNCH(ctx);
    std::vector<u64> h_flat((size_t)VW + nC);
    if (int rc = bj_memcpy_d2h(ctx, h_flat.data(), flat, h_flat.size() * 8)) return rc;
    const u64 *h_consts = h_flat.data() + VW;

    struct Term {
        unsigned k, gate, rep, term;   // k: position among the weights of its category
    };
    std::vector<Term> todo;
    const std::vector<bj::GateShape> &shapes = kind == BJ_UNSAT_GATE ? S->gates.general : S->gates.spec;
    for (unsigned g = 0; g < shapes.size(); g++) {
        const bj::GateShape &G = shapes[g];
        bool deselected = false;   // a path constant that is exactly the other bit makes this gate's selector 0 on the row
        for (unsigned b = 0; b < G.path_len; b++) deselected = deselected || h_consts[b] == (G.path[b] ? 0u : 1u);
        for (unsigned r = 0; r < G.reps && !deselected; r++)
            for (unsigned t = 0; t < G.num_terms; t++) todo.push_back({G.first_term + r * G.num_terms + t, g, r, t});
    }
    if (kind != BJ_UNSAT_GATE) {   // the specialized evaluators ADD
        BJ_HIP(ctx, hipMemsetAsync(tb, 0, todo.size() * 2 * B * 8, st));
    }
    for (size_t i = 0; i < todo.size(); i++) {
        const bj::TermSink one{d_unit + 2 * ((size_t)M - todo[i].k), B, tb + i * 2 * B, tb + i * 2 * B + B};   // the category's first power
        const bool is_general = kind == BJ_UNSAT_GATE;
        bj::launch_circuit_gates(ctx, S, bj::Cols{row_v, B}, bj::Cols{row_c, B}, is_general ? &one : nullptr, is_general ? nullptr : &one, st);
    }
    BJ_CHECK_LAUNCH(ctx);
    std::vector<u64> h_tb(todo.size() * 2 * B);
    if (!h_tb.empty())
        if (int rc = bj_memcpy_d2h(ctx, h_tb.data(), tb, h_tb.size() * 8)) return rc;
    for (size_t i = 0; i < todo.size(); i++) {
        const u64 v = gl::canon(h_tb[i * 2 * B]);
        if (!v) continue;
        out->row = row;
        out->gate = todo[i].gate;
        out->repetition = todo[i].rep;
        out->term = todo[i].term;
        out->value = v;
        return BJ_OK;
    }
    return bj::fail(ctx, BJ_ERR_HIP, "bj_check_satisfied: internal error: row %llu has a non-zero weighted sum but every term of it is zero",
                    (unsigned long long)row);
}

}  // namespace

extern "C" {

int bj_check_satisfied(bj_ctx *ctx, const bj_setup *setup, const uint64_t *d_variables, const uint64_t *d_multiplicities, bj_unsat_report *out) {
    return check_impl(ctx, setup, d_variables, d_multiplicities, out);
}

int bj_check_satisfied_from_dumps(bj_ctx *ctx, const bj_setup *setup, const void *witness_vec, size_t witness_vec_len, const void *variables_hint,
                                  size_t variables_hint_len, const void *witness_hint, size_t witness_hint_len, bj_unsat_report *out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_satisfied_from_dumps: null argument");
    return bj::witness_from_dumps(ctx, "bj_check_satisfied_from_dumps", setup, witness_vec, witness_vec_len, variables_hint, variables_hint_len,
                                  witness_hint, witness_hint_len, [&](const uint64_t *d_cells, const uint64_t *d_mult, const uint64_t *) {
                                      return check_impl(ctx, setup, d_cells, d_mult, out);
                                  });
}

}  // extern "C"
