// bj_lookup_multiplicities: the multiplicity column of a lookup argument, counted on the device from the table columns and the
// looked-up columns (what CSReferenceImplementation accumulates in lookup_multiplicities while it synthesises,
// src/cs/implementations/reference_cs.rs:54 and cs.rs:818, flattened by witness.rs:225-272).  Three kernels on the context's stream:
//   build        the index over the table rows (lookup_index.h);
//   count        one thread per (sub-argument, row): the class of its tuple gets one more, or the lookup is a miss;
//   materialise  one thread per table row: the class's count on its representative (smallest) row, 0 on every other row.
// Index, counters and miss cells live in the context's scratch (ensure_scratch); nothing here allocates, and no input is written.
#include "ctx.h"
#include "lookup_index.h"
#include "setup.h"

using gl::u64;
using namespace bj::lookup;

namespace {

// One thread per (sub-argument, row).  The adds of a wave are merged per class before they leave it: the first pending lane's
// class is broadcast, the lanes that hold the same class are balloted and served by ONE atomic of their number, and the loop
// goes on with the lanes that are left — a wave issues as many atomics as it holds distinct classes, whether one table row
// takes every lookup (unused sub-arguments) or every lane looks another row up.
__global__ void __launch_bounds__(INDEX_BLOCK) lookup_count_kernel(LookupShape L, const uint32_t *slots, unsigned long long *count, u64 *miss_min,
                                                                  u64 *miss_cnt) {
    const size_t i = (size_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
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
    bool pending = hit;
    while (pending) {
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cls);   // the first pending lane's class
        const bool mine = cls == c0;
        const u64 same = __ballot(mine);                                           // among the pending lanes
        if (mine) {
            if ((int)lane_id() == __ffsll((long long)same) - 1) atomicAdd(count + c0, (unsigned long long)__popcll(same));
            pending = false;
        }
    }
    block_min_count(live && !hit, key, miss_min, miss_cnt);
}

// one thread per table row: every word of out[0..n) is written
__global__ void __launch_bounds__(INDEX_BLOCK) lookup_materialise_kernel(LookupShape L, const uint32_t *slots, const unsigned long long *count, u64 *out) {
    const size_t r = (size_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (r >= L.n) return;
    u64 t[MAX_TUPLE];
    load_table_row(L, r, t);
    out[r] = find_class(L, slots, t) == (uint32_t)r ? (u64)count[r] : 0;   // a count is at most n * reps < 2^62: canonical
}

}  // namespace

namespace bj {

int lookup_multiplicities(bj_ctx *ctx, const char *who, const u64 *d_lvars, size_t var_stride, const u64 *d_table_id, const u64 *d_tables,
                          size_t table_stride, unsigned reps, unsigned width, unsigned log_n, u64 *d_out) {
    if (log_n > 30) return fail(ctx, BJ_ERR_UNSUPPORTED, "%s: traces above 2^30 rows (table rows are kept as 32-bit numbers)", who);
    if (width + 1 > MAX_TUPLE) return fail(ctx, BJ_ERR_UNSUPPORTED, "%s: lookup width %u above %u", who, width, MAX_TUPLE - 1);
    const size_t n = (size_t)1 << log_n;
    if ((n * reps + INDEX_BLOCK - 1) / INDEX_BLOCK > 0x7FFFFFFFull)
        return fail(ctx, BJ_ERR_UNSUPPORTED, "%s: %u sub-arguments of 2^%u rows are more lookups than one launch takes", who, reps, log_n);
    // scratch (words): 2 n 32-bit slots, n 64-bit counters, the smallest miss key and the number of misses
    if (int rc = ensure_scratch(ctx, 2 * n + 2)) return rc;
    hipStream_t st = ctx->stream;
    uint32_t *slots = (uint32_t *)ctx->d_scratch.p;
    unsigned long long *count = (unsigned long long *)(ctx->d_scratch.p + n);
    u64 *miss = ctx->d_scratch.p + 2 * n;
    BJ_HIP(ctx, hipMemsetAsync(slots, 0xFF, 2 * n * sizeof(uint32_t), st));
    BJ_HIP(ctx, hipMemsetAsync(count, 0, n * 8, st));
    const u64 miss0[2] = {NONE64, 0};
    if (int rc = h2d_async(ctx, miss, miss0, sizeof(miss0))) return rc;
    LookupShape L;
    L.tables = d_tables;
    L.lvars = d_lvars;
    L.table_id = d_table_id;
    L.n = n;
    L.tstride = table_stride;
    L.vstride = var_stride;
    L.w = width;
    L.reps = reps;
    L.cps = width + (d_table_id ? 0 : 1);
    L.mask = (uint32_t)(2 * n - 1);
    // inside a proof the two kernels are probed (bj_proof_kernel_stats); the bytes are the columns each has to read once
    const int pb = probe_begin(ctx, "lookup_index_build", 8.0 * (width + 1) * (double)n);
    hipLaunchKernelGGL(lookup_build_kernel, dim3(index_blocks(n)), dim3(INDEX_BLOCK), 0, st, L, slots);
    probe_end(ctx, pb);
    const int pc = probe_begin(ctx, "lookup_count", 8.0 * (width + 1) * (double)n * reps);
    hipLaunchKernelGGL(lookup_count_kernel, dim3(index_blocks(n * reps)), dim3(INDEX_BLOCK), 0, st, L, (const uint32_t *)slots, count, miss, miss + 1);
    probe_end(ctx, pc);
    hipLaunchKernelGGL(lookup_materialise_kernel, dim3(index_blocks(n)), dim3(INDEX_BLOCK), 0, st, L, (const uint32_t *)slots,
                       (const unsigned long long *)count, d_out);
    BJ_CHECK_LAUNCH(ctx);
    u64 h_miss[2];
    if (int rc = bj_memcpy_d2h(ctx, h_miss, miss, sizeof(h_miss))) return rc;   // synchronises
    if (h_miss[1])
        return fail(ctx, BJ_ERR_INVALID_ARG, "%s: the tuple looked up at row %llu by sub-argument %llu is in no table row (%llu such lookups)", who,
                    (unsigned long long)(h_miss[0] / reps), (unsigned long long)(h_miss[0] % reps), (unsigned long long)h_miss[1]);
    return BJ_OK;
}

int setup_lookup_multiplicities(bj_ctx *ctx, const char *who, const bj_setup *S, const u64 *d_variables, u64 *d_out) {
    const size_t n = (size_t)1 << S->log_n;
    const bj::ProofLayout &L = S->layout;
    return lookup_multiplicities(ctx, who, d_variables + (size_t)L.lookup_var(0, 0) * n, n, S->tid_var ? nullptr : S->d_nat + (size_t)L.table_id() * n,
                                 S->d_nat + (size_t)L.table(0) * n, n, S->lookup_reps, S->lookup_w, S->log_n, d_out);
}

}  // namespace bj

extern "C" {

int bj_lookup_multiplicities(bj_ctx *ctx, const uint64_t *d_lookup_vars, size_t var_stride, const uint64_t *d_table_id, const uint64_t *d_tables,
                             size_t table_stride, unsigned reps, unsigned width, unsigned log_n, uint64_t *d_multiplicities) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_lookup_vars || !d_tables || !d_multiplicities) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_multiplicities: null pointer");
    if (reps == 0 || width == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_multiplicities: bad geometry (no sub-argument, or width 0)");
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_multiplicities: a proof is running on this context");
    if (log_n <= 30 && (var_stride >> log_n) == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_multiplicities: column stride below n");
    if (log_n <= 30 && (table_stride >> log_n) == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_lookup_multiplicities: column stride below n");
    return bj::lookup_multiplicities(ctx, "bj_lookup_multiplicities", d_lookup_vars, var_stride, d_table_id, d_tables, table_stride, reps, width,
                                     log_n, d_multiplicities);
}

int bj_setup_lookup_multiplicities(bj_ctx *ctx, const bj_setup *S, const uint64_t *d_variables, uint64_t *d_multiplicities) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!S || !d_variables || !d_multiplicities) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_setup_lookup_multiplicities: null argument");
    if (S->device != ctx->device)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_setup_lookup_multiplicities: the setup lives on device %d, the context on %d", S->device, ctx->device);
    if (!S->lookup_reps) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_setup_lookup_multiplicities: the circuit has no lookups");
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_setup_lookup_multiplicities: a proof is running on this context");
    return bj::setup_lookup_multiplicities(ctx, "bj_setup_lookup_multiplicities", S, d_variables, d_multiplicities);
}

}  // extern "C"
