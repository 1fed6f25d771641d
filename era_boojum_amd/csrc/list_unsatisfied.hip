// bj_list_unsatisfied: every failure bj_check_satisfied's rule finds (include/boojum_hip_diag.h), in that call's order carried through
// to the end, truncated to the caller's capacity, with the exact totals per kind.  The rule is check_satisfied.hip's — the same
// weighted pass of the prover's evaluators flags the gate rows, the same index decides the lookups (check_shared.h) — and none of
// that file's kernels is touched.  What is added:
//   ordered compaction  count_kernel (a ballot and a popcount per wave, one number per block), block_offsets_kernel (one block:
//                       exclusive scan of the block numbers, and the running position of the list), scatter_kernel (ballot
//                       prefix inside the wave, wave prefix in LDS, block offset) — ascending, the same bytes on every run.
//                       One template over what is tested (a row's weighted sum, a term's value, a flag byte) and what is written
//                       (a row number, an entry).
//   gates               the flagged rows of a category as one ascending u32 list; then, chunk of rows by chunk, gather the rows'
//                       cells into [columns][m], evaluate every term of the category on the m rows with unit weights (T launches
//                       of launch_circuit_gates on m points: T x m, not T x n), and compact the non-zero (row, term) items
//                       straight into entries.  Every chunk adds its number to the kind's total; the scatter drops what lies past
//                       the capacity, so the chunks behind the first only count.
//   lookups             variants of the probe and compare kernels that leave one flag byte per (row, sub-argument) and per table
//                       row, compacted into entries behind the gates' ones.
// The position of the list, the four totals and the two numbers of flagged rows live in eight words of scratch; the host reads
// the numbers of flagged rows once (they size the chunk loops) and the totals and entries once at the end.
#include "../../include/boojum_hip_diag.h"
#include "check_shared.h"
#include "ctx.h"
#include "list_plan.h"
#include "lookup_index.h"
#include "setup.h"

#include <cstring>
#include <vector>

using gl::u64;
using namespace bj::lookup;
using namespace bj::check;

namespace {

static_assert(bj::LIST_BLOCK == CHECK_BLOCK && bj::LIST_BLOCK % 64 == 0, "one block size behind both files, whole waves");
constexpr unsigned LB = bj::LIST_BLOCK, WAVES = LB / 64;
static_assert(sizeof(bj_unsat_entry) == 40, "five words per entry");

// words of the device state
enum { ST_POS = 0, ST_TOTAL = 0 /* + kind */, ST_ROWS = 5 /* + category */, ST_BASE = 7, ST_WORDS = 8 };

// ---- what is tested
struct RowNonzero {   // a row whose weighted sum of terms is not zero (check_satisfied.hip's nonzero_rows_kernel)
    const u64 *t0, *t1;
    __device__ bool operator()(size_t i) const { return (gl::canon(t0[i]) | gl::canon(t1[i])) != 0; }
};
struct TermNonzero {   // item j * T + k: term k on row j of the chunk, its value at tb[k][0][j]
    const u64 *tb;
    size_t m;
    unsigned T;
    __device__ bool operator()(size_t i) const {
        const size_t j = i / T, k = i - j * T;
        return gl::canon(tb[k * 2 * m + j]) != 0;
    }
};
struct FlagSet {
    const uint8_t *flag;
    __device__ bool operator()(size_t i) const { return flag[i] != 0; }
};

// ---- what is written at position pos for item i
struct RowOut {
    uint32_t *list;
    __device__ void operator()(u64 pos, size_t i) const { list[pos] = (uint32_t)i; }
};
__device__ __forceinline__ void put_entry(bj_unsat_entry *e, uint32_t kind, uint32_t gate, uint32_t rep, uint32_t term, u64 row, u64 value, u64 expected) {
    e->kind = kind; e->gate = gate; e->repetition = rep; e->term = term;
    e->row = row; e->value = value; e->expected = expected;
}
struct TermOut {
    bj_unsat_entry *entries;
    const u64 *tb;
    size_t m;
    unsigned T;
    const uint32_t *info;   // [T][3]: gate, repetition, term
    const uint32_t *rows;   // the chunk's rows
    uint32_t kind;
    __device__ void operator()(u64 pos, size_t i) const {
        const size_t j = i / T, k = i - j * T;
        put_entry(entries + pos, kind, info[3 * k], info[3 * k + 1], info[3 * k + 2], rows[j], gl::canon(tb[k * 2 * m + j]), 0);
    }
};
struct LookupOut {   // item row * reps + sub-argument
    bj_unsat_entry *entries;
    unsigned reps;
    __device__ void operator()(u64 pos, size_t i) const { put_entry(entries + pos, BJ_UNSAT_LOOKUP, (uint32_t)(i % reps), 0, 0, i / reps, 0, 0); }
};
struct ClassOut {    // item: the class's smallest table row
    bj_unsat_entry *entries;
    const unsigned long long *count, *lo;
    const uint32_t *hi;
    __device__ void operator()(u64 pos, size_t i) const { put_entry(entries + pos, BJ_UNSAT_MULTIPLICITY, 0, 0, 0, i, count[i], expected_value(lo[i], hi[i])); }
};

// ---- ordered compaction
template <class Test>
__global__ void __launch_bounds__(LB) count_kernel(Test test, size_t items, uint32_t *block_count) {
    __shared__ unsigned s_cnt[WAVES];
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    const bool hit = i < items && test(i);
    const unsigned cnt = (unsigned)__popcll(__ballot(hit));
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0;
#pragma unroll
        for (unsigned w = 0; w < WAVES; w++) c += s_cnt[w];
        block_count[blockIdx.x] = c;
    }
}

// ONE block: block_offset[b] = sum of block_count[0..b); then *base = *pos, *pos += the sum, *accum (if any) += the sum
__global__ void __launch_bounds__(LB) block_offsets_kernel(const uint32_t *block_count, size_t blocks, u64 *block_offset, u64 *pos, u64 *accum, u64 *base) {
    __shared__ u64 s_wave[WAVES];
    __shared__ u64 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (size_t b0 = 0; b0 < blocks; b0 += LB) {
        const size_t b = b0 + threadIdx.x;
        const u64 c = b < blocks ? block_count[b] : 0;
        u64 incl = c;
#pragma unroll
        for (unsigned d = 1; d < 64; d <<= 1) {
            const u64 o = __shfl_up(incl, d);
            if (lane_id() >= d) incl += o;
        }
        if (lane_id() == 63) s_wave[threadIdx.x >> 6] = incl;
        __syncthreads();
        u64 before = s_carry;
        for (unsigned w = 0; w < (threadIdx.x >> 6); w++) before += s_wave[w];
        if (b < blocks) block_offset[b] = before + incl - c;
        __syncthreads();
        if (threadIdx.x == LB - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const u64 total = s_carry, at = *pos;
        *base = at;
        *pos = at + total;
        if (accum) *accum += total;
    }
}

// item i goes to position *base + (hits before it); positions from `limit` on are dropped
template <class Test, class Out>
__global__ void __launch_bounds__(LB) scatter_kernel(Test test, Out out, size_t items, const u64 *block_offset, const u64 *base, u64 limit) {
    __shared__ unsigned s_cnt[WAVES];
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    const bool hit = i < items && test(i);
    const u64 hits = __ballot(hit);
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = (unsigned)__popcll(hits);
    __syncthreads();
    if (!hit) return;
    u64 pos = *base + block_offset[blockIdx.x] + (u64)__popcll(hits & (((u64)1 << lane_id()) - 1));
    for (unsigned w = 0; w < (threadIdx.x >> 6); w++) pos += s_cnt[w];
    if (pos < limit) out(pos, i);
}

struct Compactor {
    bj_ctx *ctx;
    uint32_t *block_count;
    u64 *block_offset, *state;
    // the hits among `items` items, in ascending order, from position *pos on (which moves past them); *accum += their number
    template <class Test, class Out>
    void run(Test test, Out out, size_t items, u64 *pos, u64 *accum, u64 limit) const {
        const unsigned blocks = blocks_for(items);
        hipStream_t st = ctx->stream;
        if (blocks) hipLaunchKernelGGL(HIP_KERNEL_NAME(count_kernel<Test>), dim3(blocks), dim3(LB), 0, st, test, items, block_count);
        hipLaunchKernelGGL(block_offsets_kernel, dim3(1), dim3(LB), 0, st, (const uint32_t *)block_count, (size_t)blocks, block_offset, pos, accum, state + ST_BASE);
        if (blocks)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(scatter_kernel<Test, Out>), dim3(blocks), dim3(LB), 0, st, test, out, items, (const u64 *)block_offset,
                               (const u64 *)(state + ST_BASE), limit);
    }
};

// out[c][j] = canonical src[c][rows[j]] for j < count, 0 for the padding up to m
__global__ void __launch_bounds__(LB) gather_rows_kernel(const u64 *src, size_t stride, const uint32_t *rows, size_t count, size_t m, u64 *out) {
    const size_t j = (size_t)blockIdx.x * LB + threadIdx.x, c = blockIdx.y;
    if (j >= m) return;
    out[c * m + j] = j < count ? gl::canon(src[c * stride + rows[j]]) : 0;
}

// lookup_probe_kernel of check_satisfied.hip with one flag byte per item instead of the first miss: flag[row * reps + sub]
__global__ void __launch_bounds__(LB) lookup_probe_flag_kernel(LookupShape L, const uint32_t *slots, unsigned long long *count, uint8_t *flag) {
    const size_t i = (size_t)blockIdx.x * LB + threadIdx.x;
    const bool live = i < L.n * L.reps;
    uint32_t cls = SLOT_EMPTY;
    size_t key = 0;
    if (live) {
        const size_t sub = i / L.n, row = i - sub * L.n;
        u64 t[MAX_TUPLE];
        load_looked_up(L, sub, row, t);
        cls = find_class(L, slots, t);
        key = row * L.reps + sub;
    }
    const bool hit = live && cls != SLOT_EMPTY;
    const u64 hits = __ballot(hit);
    if (hits) {
        const int leader = __ffsll((long long)hits) - 1;
        const uint32_t c0 = __shfl(cls, leader);
        const u64 same = __ballot(hit && cls == c0);
        if ((int)lane_id() == leader) atomicAdd(count + c0, (unsigned long long)__popcll(same));
        if (hit && cls != c0) atomicAdd(count + cls, 1ull);
    }
    if (live) flag[key] = hit ? 0 : 1;
}

// lookup_compare_kernel of check_satisfied.hip with one flag byte per table row
__global__ void __launch_bounds__(LB) lookup_compare_flag_kernel(size_t n, const uint32_t *class_of, const unsigned long long *count,
                                                                 const unsigned long long *lo, const uint32_t *hi, uint8_t *flag) {
    const size_t r = (size_t)blockIdx.x * LB + threadIdx.x;
    if (r >= n) return;
    flag[r] = class_of[r] == (uint32_t)r && expected_value(lo[r], hi[r]) != (u64)count[r];
}

int list_impl(bj_ctx *ctx, const bj_setup *S, const u64 *d_variables, const u64 *d_multiplicities, bj_unsat_entry *h_entries, size_t capacity,
              size_t *n_entries, uint64_t *totals) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!S || !d_variables || !n_entries || !totals || (!h_entries && capacity)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_list_unsatisfied: null argument");
    if (S->device != ctx->device) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_list_unsatisfied: the setup lives on device %d, the context on %d", S->device, ctx->device);
    const bool has_lookup = S->lookup_reps > 0;
    if (has_lookup && !d_multiplicities) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_list_unsatisfied: multiplicities required");
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_list_unsatisfied: a proof is running on this context");
    if (S->log_n > 30) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_list_unsatisfied: traces above 2^30 rows (table rows are kept as 32-bit numbers)");
    if (has_lookup && S->lookup_w + 1 > MAX_TUPLE) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_list_unsatisfied: lookup width %u above %u", S->lookup_w, MAX_TUPLE - 1);
    *n_entries = 0;
    std::memset(totals, 0, 5 * sizeof(uint64_t));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)1 << S->log_n;
    const bj::ProofLayout &PL = S->layout;
    const unsigned VW = S->V + S->Wc, nC = S->nC, reps = S->lookup_reps;
    const u64 *d_consts = S->d_nat + (size_t)PL.constant(0) * n;

    // terms in evaluator order, as in check_satisfied.hip; per category the (gate, repetition, term) of every term
    const unsigned n_cat[2] = {S->gates.n_general_terms, S->gates.n_spec_terms}, n_terms = n_cat[0] + n_cat[1];
    const unsigned T_max = n_cat[0] > n_cat[1] ? n_cat[0] : n_cat[1], M = T_max + 1;
    std::vector<uint32_t> info(3 * (size_t)n_terms + 2, 0);
    unsigned max_general = 0;
    for (int cat = 0; cat < 2; cat++) {
        const std::vector<bj::GateShape> &shapes = cat ? S->gates.spec : S->gates.general;
        for (unsigned g = 0; g < shapes.size(); g++) {
            const bj::GateShape &G = shapes[g];
            if (!cat && G.terms() > max_general) max_general = G.terms();
            for (unsigned r = 0; r < G.reps; r++)
                for (unsigned t = 0; t < G.num_terms; t++) {
                    uint32_t *p = info.data() + 3 * ((size_t)(cat ? n_cat[0] : 0) + G.first_term + (size_t)r * G.num_terms + t);
                    p[0] = g; p[1] = r; p[2] = t;
                }
        }
    }
    const size_t m = (size_t)bj::list_chunk_rows(capacity, n);
    const size_t slots = (size_t)bj::list_entry_slots(capacity, n, max_general, n_cat[1], reps);
    size_t max_items = n > m * T_max ? n : m * T_max;
    if (n * reps > max_items) max_items = n * reps;
    const size_t max_blocks = blocks_for(max_items);

    // scratch layout (words)
    size_t off = 0;
    auto take = [&off](size_t words) {
        const size_t at = off;
        off += (words + 1) & ~(size_t)1;
        return at;
    };
    const size_t o_t = take(2 * n), o_state = take(ST_WORDS), o_alpha = take(2 * (size_t)n_terms + 2), o_unit = take(2 * (2 * (size_t)M + 1));
    const size_t o_info = take(info.size() / 2 + 1), o_rows0 = take(n_cat[0] ? n / 2 + 1 : 0), o_rows1 = take(n_cat[1] ? n / 2 + 1 : 0);
    const size_t o_bcnt = take(max_blocks / 2 + 1), o_boff = take(max_blocks + 1);
    const size_t o_cols_v = take((size_t)VW * m), o_cols_c = take((size_t)nC * m), o_tb = take((size_t)T_max * 2 * m);
    const size_t o_slots = has_lookup ? take(n) : 0, o_count = has_lookup ? take(n) : 0, o_lo = has_lookup ? take(n) : 0;
    const size_t o_hi = has_lookup ? take(n / 2 + 1) : 0, o_cls = has_lookup ? take(n / 2 + 1) : 0;
    const size_t o_flag3 = has_lookup ? take(n * reps / 8 + 1) : 0, o_flag4 = has_lookup ? take(n / 8 + 1) : 0;
    const size_t o_entries = take(slots * (sizeof(bj_unsat_entry) / 8));
    if (int rc = bj::ensure_scratch(ctx, off)) return rc;
    u64 *W = ctx->d_scratch.p;
    u64 *t0 = W + o_t, *t1 = t0 + n, *state = W + o_state, *d_alpha = W + o_alpha, *d_unit = W + o_unit;
    const uint32_t *d_info = (const uint32_t *)(W + o_info);
    uint32_t *d_rows[2] = {(uint32_t *)(W + o_rows0), (uint32_t *)(W + o_rows1)};
    bj_unsat_entry *d_entries = (bj_unsat_entry *)(W + o_entries);
    const Compactor compact{ctx, (uint32_t *)(W + o_bcnt), W + o_boff, state};

    {
        const u64 zero[ST_WORDS] = {};
        if (int rc = bj::h2d_async(ctx, state, zero, sizeof(zero))) return rc;
        std::vector<u64> alphas(2 * (size_t)n_terms + 2, 0);
        u64 seed = ALPHA_SEED;
        for (size_t i = 0; i < 2 * (size_t)n_terms; i++) alphas[i] = splitmix64(seed) % gl::P;
        if (int rc = bj::h2d_async(ctx, d_alpha, alphas.data(), alphas.size() * 8)) return rc;
        std::vector<u64> unit(2 * (2 * (size_t)M + 1), 0);
        unit[2 * (size_t)M] = 1;   // seen from d_unit + 2 * (M - k), term k has weight (1, 0) and every other term (0, 0)
        if (int rc = bj::h2d_async(ctx, d_unit, unit.data(), unit.size() * 8)) return rc;
        if (int rc = bj::h2d_async(ctx, W + o_info, info.data(), info.size() * 4)) return rc;
    }

    // ---- the flagged rows of both categories: check_satisfied.hip's phase 1, then the rows as ascending lists
    const bj::Cols trace_vars{d_variables, n}, trace_consts{d_consts, n};
    const bj::TermSink general{d_alpha, n, t0, t1}, spec{d_alpha + 2 * (size_t)n_cat[0], n, t0, t1};
    if (n_cat[0]) {
        bj::launch_circuit_gates(ctx, S, trace_vars, trace_consts, &general, nullptr, st);
        compact.run(RowNonzero{t0, t1}, RowOut{d_rows[0]}, n, state + ST_ROWS + 0, nullptr, n);
    }
    if (n_cat[1]) {
        BJ_HIP(ctx, hipMemsetAsync(t0, 0, 2 * n * 8, st));
        bj::launch_circuit_gates(ctx, S, trace_vars, trace_consts, nullptr, &spec, st);
        compact.run(RowNonzero{t0, t1}, RowOut{d_rows[1]}, n, state + ST_ROWS + 1, nullptr, n);
    }
    BJ_CHECK_LAUNCH(ctx);

    // ---- lookups: counts per class, a flag per (row, sub-argument) and per table row
    unsigned long long *d_count = nullptr, *d_lo = nullptr;
    uint32_t *d_hi = nullptr;
    uint8_t *flag3 = nullptr, *flag4 = nullptr;
    if (has_lookup) {
        uint32_t *slots_tab = (uint32_t *)(W + o_slots), *class_of = (uint32_t *)(W + o_cls);
        d_count = (unsigned long long *)(W + o_count);
        d_lo = (unsigned long long *)(W + o_lo);
        d_hi = (uint32_t *)(W + o_hi);
        flag3 = (uint8_t *)(W + o_flag3);
        flag4 = (uint8_t *)(W + o_flag4);
        BJ_HIP(ctx, hipMemsetAsync(slots_tab, 0xFF, 2 * n * sizeof(uint32_t), st));
        BJ_HIP(ctx, hipMemsetAsync(d_count, 0, n * 8, st));
        BJ_HIP(ctx, hipMemsetAsync(d_lo, 0, n * 8, st));
        BJ_HIP(ctx, hipMemsetAsync(d_hi, 0, n * 4, st));
        LookupShape L;
        L.tables = S->d_nat + (size_t)PL.table(0) * n;
        L.lvars = d_variables + (size_t)PL.lookup_var(0, 0) * n;
        L.table_id = S->tid_var ? nullptr : S->d_nat + (size_t)PL.table_id() * n;
        L.n = L.tstride = L.vstride = n;
        L.w = S->lookup_w;
        L.reps = reps;
        L.cps = S->lookup_cps;
        L.mask = (uint32_t)(2 * n - 1);
        hipLaunchKernelGGL(lookup_build_kernel, dim3(blocks_for(n)), dim3(LB), 0, st, L, slots_tab);
        hipLaunchKernelGGL(lookup_probe_flag_kernel, dim3(blocks_for(n * reps)), dim3(LB), 0, st, L, (const uint32_t *)slots_tab, d_count, flag3);
        hipLaunchKernelGGL(lookup_expected_kernel, dim3(blocks_for(n)), dim3(LB), 0, st, L, (const uint32_t *)slots_tab, d_multiplicities, class_of, d_lo, d_hi);
        hipLaunchKernelGGL(lookup_compare_flag_kernel, dim3(blocks_for(n)), dim3(LB), 0, st, n, (const uint32_t *)class_of, (const unsigned long long *)d_count,
                           (const unsigned long long *)d_lo, (const uint32_t *)d_hi, flag4);
        BJ_CHECK_LAUNCH(ctx);
    }

    // ---- gates: every term on the flagged rows, chunk by chunk (the numbers of flagged rows size the loops)
    u64 h_state[ST_WORDS];
    if (n_terms) {
        if (int rc = bj_memcpy_d2h(ctx, h_state, state, sizeof(h_state))) return rc;   // synchronises
    } else {
        std::memset(h_state, 0, sizeof(h_state));
    }
    u64 *cols_v = W + o_cols_v, *cols_c = W + o_cols_c, *tb = W + o_tb;
    for (int cat = 0; cat < 2; cat++) {
        const size_t flagged = (size_t)h_state[ST_ROWS + cat];
        const unsigned T = n_cat[cat];
        const uint32_t kind = cat ? BJ_UNSAT_SPECIALIZED_GATE : BJ_UNSAT_GATE;
        const uint32_t *cat_info = d_info + 3 * (size_t)(cat ? n_cat[0] : 0);
        for (size_t c = 0; c < (size_t)bj::list_chunks(flagged, m); c++) {
            const uint32_t *rows = d_rows[cat] + c * m;
            const size_t count = flagged - c * m < m ? flagged - c * m : m;
            hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks_for(m), VW), dim3(LB), 0, st, d_variables, n, rows, count, m, cols_v);
            if (nC) hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks_for(m), nC), dim3(LB), 0, st, d_consts, n, rows, count, m, cols_c);
            if (cat) BJ_HIP(ctx, hipMemsetAsync(tb, 0, (size_t)T * 2 * m * 8, st));   // the specialized evaluators ADD
            for (unsigned k = 0; k < T; k++) {
                const bj::TermSink one{d_unit + 2 * ((size_t)M - k), m, tb + (size_t)k * 2 * m, tb + (size_t)k * 2 * m + m};
                bj::launch_circuit_gates(ctx, S, bj::Cols{cols_v, m}, bj::Cols{cols_c, m}, cat ? nullptr : &one, cat ? &one : nullptr, st);
            }
            compact.run(TermNonzero{tb, m, T}, TermOut{d_entries, tb, m, T, cat_info, rows, kind}, count * T, state + ST_POS, state + ST_TOTAL + kind, slots);
            BJ_CHECK_LAUNCH(ctx);
        }
    }
    if (has_lookup) {
        compact.run(FlagSet{flag3}, LookupOut{d_entries, reps}, n * reps, state + ST_POS, state + ST_TOTAL + BJ_UNSAT_LOOKUP, slots);
        compact.run(FlagSet{flag4}, ClassOut{d_entries, d_count, d_lo, d_hi}, n, state + ST_POS, state + ST_TOTAL + BJ_UNSAT_MULTIPLICITY, slots);
        BJ_CHECK_LAUNCH(ctx);
    }

    // ---- to the host: the totals, then the entries in one copy
    if (int rc = bj_memcpy_d2h(ctx, h_state, state, sizeof(h_state))) return rc;   // synchronises
    uint64_t by_kind[5] = {0, h_state[1], h_state[2], h_state[3], h_state[4]};
    const bj::ListSplit split = bj::list_split(capacity, by_kind);
    if (split.total != h_state[ST_POS] || split.kept > slots)
        return bj::fail(ctx, BJ_ERR_HIP, "bj_list_unsatisfied: internal error: the list ends at %llu, its kinds sum to %llu", (unsigned long long)h_state[ST_POS],
                        (unsigned long long)split.total);
    if ((h_state[ST_ROWS + 0] && !by_kind[1]) || (h_state[ST_ROWS + 1] && !by_kind[2]))
        return bj::fail(ctx, BJ_ERR_HIP, "bj_list_unsatisfied: internal error: a row has a non-zero weighted sum but every term of it is zero");
    if (split.kept)
        if (int rc = bj_memcpy_d2h(ctx, h_entries, d_entries, (size_t)split.kept * sizeof(bj_unsat_entry))) return rc;
    for (int k = 1; k <= 4; k++)
        if (split.written[k] && h_entries[split.first[k]].kind != (uint32_t)k)
            return bj::fail(ctx, BJ_ERR_HIP, "bj_list_unsatisfied: internal error: entry %llu is not the first of kind %d", (unsigned long long)split.first[k], k);
    totals[0] = split.total;
    for (int k = 1; k <= 4; k++) totals[k] = by_kind[k];
    *n_entries = (size_t)split.kept;
    return BJ_OK;
}

}  // namespace

extern "C" {

int bj_list_unsatisfied(bj_ctx *ctx, const bj_setup *setup, const uint64_t *d_variables, const uint64_t *d_multiplicities, bj_unsat_entry *h_entries,
                        size_t capacity, size_t *n_entries, uint64_t totals[5]) {
    return list_impl(ctx, setup, d_variables, d_multiplicities, h_entries, capacity, n_entries, totals);
}

int bj_list_unsatisfied_from_dumps(bj_ctx *ctx, const bj_setup *setup, const void *witness_vec, size_t witness_vec_len, const void *variables_hint,
                                   size_t variables_hint_len, const void *witness_hint, size_t witness_hint_len, bj_unsat_entry *h_entries,
                                   size_t capacity, size_t *n_entries, uint64_t totals[5]) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!n_entries || !totals || (!h_entries && capacity)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_list_unsatisfied_from_dumps: null argument");
    return bj::witness_from_dumps(ctx, "bj_list_unsatisfied_from_dumps", setup, witness_vec, witness_vec_len, variables_hint, variables_hint_len,
                                  witness_hint, witness_hint_len, [&](const uint64_t *d_cells, const uint64_t *d_mult, const uint64_t *) {
                                      return list_impl(ctx, setup, d_cells, d_mult, h_entries, capacity, n_entries, totals);
                                  });
}

}  // extern "C"
