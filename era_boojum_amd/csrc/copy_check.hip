// bj_sigma_cells / bj_check_copy_constraints: which cells break a copy constraint.  The inverse of setup_placement.hip: a sigma
// value k_j * omega^r (create_permutation_polys, src/cs/implementations/setup.rs:419-503) is turned back into the cell (j, r) it
// names, and the copy-permutation argument's claim (src/cs/implementations/copy_permutation.rs) — sigma is a permutation of the
// cells and every cell holds the value of the cell its sigma names — is tested cell by cell instead of by a grand product.
//
// Decoding one word, one lane per cell (consecutive lanes = consecutive rows of one column):
//   column  s = sigma^n (log_n squarings) is k_j^n exactly when sigma lies in k_j * H (H: the n-th roots of unity), so s is
//           looked up by binary search in the sorted list of the k_j^n, staged in LDS once per block; 0 is in no coset.
//   row     y = sigma / k_j is in H; Pohlig-Hellman in the plain form, WINDOW = 4 bits per round: with r known below bit i and
//           y = omega^(r - (r mod 2^i)), t = y^(2^(log_n - i - w)) is the 2^w-th root of unity rho_w^b, b = bits [i, i + w) of r;
//           b is found by comparing t with the 16 powers of the 16th root (rho_w^b = rho_4^(b << (4 - w))), then
//           y *= omega^-(b << i) from a 16-entry list per round.  Both lists are wave-uniform LDS reads; nothing is gathered.
//   Products per cell: log_n squarings, one product, then (log_n - 4) + (log_n - 8) + ... squarings and one product per round:
//   79 at log_n = 22 (the bit-by-bit form needs 22 + 1 + 231 + 22).
// The decoder is one __host__ __device__ function: the host decodes the single cell a report names with the code the kernel ran.
#include "ctx.h"
#include "lookup_index.h"
#include "setup.h"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

using gl::u64;
using bj::lookup::block_min_count;
using bj::lookup::NONE64;

namespace {

constexpr unsigned COPY_BLOCK = bj::lookup::INDEX_BLOCK;
constexpr unsigned WINDOW = 4, WINDOW_VALUES = 1u << WINDOW, MAX_ROUNDS = 8;   // 8 rounds of 4 bits cover log_n <= 30
constexpr unsigned TAIL_WORDS = WINDOW_VALUES + MAX_ROUNDS * WINDOW_VALUES;   // roots, then steps
constexpr uint32_t NO_CELL = 0xFFFFFFFFu;
constexpr unsigned MAX_COLUMNS = 4096;   // the sorted k_j^n of every column sit in LDS (8 bytes per column)

// The decoding table, u64 words: keys[V] (k_j^n, ascending) | kinv[V] (1 / k_j, in key order) | col[V] (j, in key order) |
// roots[16] (rho_4^b) | steps[MAX_ROUNDS][16] (omega^-(b << 4 * round)).  The kernels stage keys, roots and steps in LDS.
struct TableView {
    const u64 *keys, *kinv, *col, *roots, *steps;
};
inline size_t table_words(unsigned V) { return 3 * (size_t)V + TAIL_WORDS; }

// canonical sigma word -> cell number j * n + r, NO_CELL if it lies in no coset.  No early exit: a lane whose word is in no
// coset runs the same products on garbage, so that the waves of the kernels stay converged.
__host__ __device__ __forceinline__ uint32_t decode_cell(u64 sigma, unsigned V, unsigned log_n, const TableView &T) {
    u64 s = sigma;
    for (unsigned i = 0; i < log_n; i++) s = gl::sqr(s);
    unsigned lo = 0, hi = V;   // first position whose key is not below s
    while (lo < hi) {
        const unsigned mid = (lo + hi) / 2;
        if (T.keys[mid] < s)
            lo = mid + 1;
        else
            hi = mid;
    }
    const unsigned at = lo < V ? lo : V - 1;
    bool ok = T.keys[at] == s;
    u64 y = gl::mul(sigma, T.kinv[at]);
    uint32_t r = 0;
    for (unsigned i = 0, round = 0; i < log_n; i += WINDOW, round++) {
        const unsigned w = log_n - i < WINDOW ? log_n - i : WINDOW;
        u64 t = y;
        for (unsigned e = log_n - i - w; e > 0; e--) t = gl::sqr(t);
        unsigned b = WINDOW_VALUES;
        for (unsigned x = 0; x < (1u << w); x++)
            if (T.roots[x << (WINDOW - w)] == t) b = x;
        if (b == WINDOW_VALUES) {   // y is not in H: only behind a failed column search
            ok = false;
            b = 0;
        }
        y = gl::mul(y, T.steps[round * WINDOW_VALUES + b]);
        r |= b << i;
    }
    return ok ? ((uint32_t)T.col[at] << log_n) | r : NO_CELL;
}

// keys, roots and steps into LDS; `lds` holds V + TAIL_WORDS words
__device__ __forceinline__ TableView stage_table(const u64 *table, unsigned V, u64 *lds) {
    for (unsigned i = threadIdx.x; i < V; i += COPY_BLOCK) lds[i] = table[i];
    for (unsigned i = threadIdx.x; i < TAIL_WORDS; i += COPY_BLOCK) lds[V + i] = table[3 * (size_t)V + i];
    __syncthreads();
    return {lds, table + V, table + 2 * (size_t)V, lds + V, lds + V + WINDOW_VALUES};
}

// ctr: [0] smallest key (row * V + column) of a word in no coset, [1] their number
__global__ void __launch_bounds__(COPY_BLOCK) sigma_cells_kernel(const u64 *sigmas, size_t sig_stride, unsigned V, unsigned log_n, const u64 *table,
                                                                uint32_t *cells, size_t cell_stride, u64 *ctr) {
    extern __shared__ u64 lds[];
    const TableView T = stage_table(table, V, lds);
    const size_t i = (size_t)blockIdx.x * COPY_BLOCK + threadIdx.x, row_mask = ((size_t)1 << log_n) - 1;
    const bool live = i < ((size_t)V << log_n);
    const size_t c = i >> log_n, row = i & row_mask;
    const u64 sigma = live ? gl::canon(sigmas[c * sig_stride + row]) : 0;
    const uint32_t cell = decode_cell(sigma, V, log_n, T);
    if (live) cells[c * cell_stride + row] = cell;
    block_min_count(live && cell == NO_CELL, (u64)row * V + c, ctr + 0, ctr + 1);
}

// One pass over the cells of a setup ([V][n] sigmas and variables, both at stride n).  ctr: [0], [1] words in no coset (smallest
// key, number); [3] sigma entries whose target was already marked in `seen` (such a target is marked in `multi` as well); [4],
// [5] cells whose canonical value differs from that of the cell their sigma names.  [2] is left to the second pass.
__global__ void __launch_bounds__(COPY_BLOCK) copy_check_kernel(const u64 *sigmas, const u64 *vars, unsigned V, unsigned log_n, const u64 *table,
                                                               uint32_t *seen, uint32_t *multi, u64 *ctr) {
    extern __shared__ u64 lds[];
    const TableView T = stage_table(table, V, lds);
    const size_t i = (size_t)blockIdx.x * COPY_BLOCK + threadIdx.x, row_mask = ((size_t)1 << log_n) - 1;
    const bool live = i < ((size_t)V << log_n);
    const size_t c = i >> log_n, row = i & row_mask;
    const u64 key = (u64)row * V + c;
    const uint32_t cell = decode_cell(live ? gl::canon(sigmas[i]) : 0, V, log_n, T);
    const bool named = live && cell != NO_CELL;
    bool again = false, differs = false;
    if (named) {
        const uint32_t bit = 1u << (cell & 31);
        again = (atomicOr(seen + (cell >> 5), bit) & bit) != 0;
        if (again) atomicOr(multi + (cell >> 5), bit);
        differs = gl::canon(vars[i]) != gl::canon(vars[cell]);
    }
    block_min_count(live && !named, key, ctr + 0, ctr + 1);
    __syncthreads();   // block_min_count's LDS words are reused by the next call
    block_min_count(again, NONE64, ctr + 2, ctr + 3);
    __syncthreads();
    block_min_count(differs, key, ctr + 4, ctr + 5);
}

// Second pass, only when [3] != 0: the smallest key among the sigma entries whose target another entry names too (a target
// marked in `multi`), whatever order the atomics of the first pass landed in.  ctr[2] smallest key; ctr[6] takes the number.
__global__ void __launch_bounds__(COPY_BLOCK) copy_shared_target_kernel(const u64 *sigmas, unsigned V, unsigned log_n, const u64 *table,
                                                                       const uint32_t *multi, u64 *ctr) {
    extern __shared__ u64 lds[];
    const TableView T = stage_table(table, V, lds);
    const size_t i = (size_t)blockIdx.x * COPY_BLOCK + threadIdx.x, row_mask = ((size_t)1 << log_n) - 1;
    const bool live = i < ((size_t)V << log_n);
    const size_t c = i >> log_n, row = i & row_mask;
    const uint32_t cell = decode_cell(live ? gl::canon(sigmas[i]) : 0, V, log_n, T);
    const bool shared = live && cell != NO_CELL && ((multi[cell >> 5] >> (cell & 31)) & 1u);
    block_min_count(shared, (u64)row * V + c, ctr + 2, ctr + 6);
}

unsigned blocks_for(size_t items) { return (unsigned)((items + COPY_BLOCK - 1) / COPY_BLOCK); }
size_t lds_bytes(unsigned V) { return ((size_t)V + TAIL_WORDS) * sizeof(u64); }

// The limits of both entry points, then the table on the host.  Nothing is launched or read from the device here.
int build_table(bj_ctx *ctx, const char *who, const u64 *h_non_residues, unsigned V, unsigned log_n, std::vector<u64> &t) {
    if (V == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: no columns", who);
    if (log_n > 30) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "%s: log_n %u > 30 not supported", who, log_n);
    if (((u64)V << log_n) >= ((u64)1 << 32))
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "%s: %u columns of 2^%u rows: cell numbers must fit 32 bits (num_vars * n < 2^32)", who, V, log_n);
    if (V > MAX_COLUMNS) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "%s: %u columns, at most %u are supported", who, V, MAX_COLUMNS);
    std::vector<u64> kn(V), k(V);
    for (unsigned j = 0; j < V; j++) {
        k[j] = gl::canon(h_non_residues[j]);
        if (!k[j]) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: non-residue %u is 0", who, j);
        kn[j] = k[j];
        for (unsigned i = 0; i < log_n; i++) kn[j] = gl::sqr(kn[j]);
    }
    std::vector<unsigned> order(V);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return kn[a] != kn[b] ? kn[a] < kn[b] : a < b; });
    for (unsigned p = 1; p < V; p++)
        if (kn[order[p]] == kn[order[p - 1]])
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: non-residues %u and %u name the same coset (k^n is equal)", who, order[p - 1], order[p]);
    t.assign(table_words(V), 0);
    for (unsigned p = 0; p < V; p++) {
        t[p] = kn[order[p]];
        t[V + p] = gl::inv(k[order[p]]);
        t[2 * (size_t)V + p] = order[p];
    }
    u64 *roots = t.data() + 3 * (size_t)V, *steps = roots + WINDOW_VALUES;
    const u64 rho = gl::omega(WINDOW), omega_inv = gl::inv(gl::omega(log_n));
    roots[0] = 1;
    for (unsigned b = 1; b < WINDOW_VALUES; b++) roots[b] = gl::mul(roots[b - 1], rho);
    u64 base = omega_inv;   // omega^-(2^(4 * round))
    for (unsigned round = 0; round < MAX_ROUNDS; round++) {
        steps[round * WINDOW_VALUES] = 1;
        for (unsigned b = 1; b < WINDOW_VALUES; b++) steps[round * WINDOW_VALUES + b] = gl::mul(steps[round * WINDOW_VALUES + b - 1], base);
        for (unsigned i = 0; i < WINDOW; i++) base = gl::sqr(base);
    }
    return BJ_OK;
}

TableView host_view(const std::vector<u64> &t, unsigned V) {
    const u64 *p = t.data();
    return {p, p + V, p + 2 * (size_t)V, p + 3 * (size_t)V, p + 3 * (size_t)V + WINDOW_VALUES};
}

}  // namespace

namespace bj {

void launch_sigma_cells(const u64 *d_sigmas, size_t sig_stride, unsigned num_vars, unsigned log_n, const u64 *d_table, uint32_t *d_cells,
                        size_t cell_stride, u64 *d_ctr, hipStream_t s) {
    hipLaunchKernelGGL(sigma_cells_kernel, dim3(blocks_for((size_t)num_vars << log_n)), dim3(COPY_BLOCK), lds_bytes(num_vars), s, d_sigmas, sig_stride,
                       num_vars, log_n, d_table, d_cells, cell_stride, d_ctr);
}
void launch_copy_check(const u64 *d_sigmas, const u64 *d_vars, unsigned num_vars, unsigned log_n, const u64 *d_table, uint32_t *d_seen,
                       uint32_t *d_multi, u64 *d_ctr, hipStream_t s) {
    hipLaunchKernelGGL(copy_check_kernel, dim3(blocks_for((size_t)num_vars << log_n)), dim3(COPY_BLOCK), lds_bytes(num_vars), s, d_sigmas, d_vars,
                       num_vars, log_n, d_table, d_seen, d_multi, d_ctr);
}
void launch_copy_shared_target(const u64 *d_sigmas, unsigned num_vars, unsigned log_n, const u64 *d_table, const uint32_t *d_multi, u64 *d_ctr,
                               hipStream_t s) {
    hipLaunchKernelGGL(copy_shared_target_kernel, dim3(blocks_for((size_t)num_vars << log_n)), dim3(COPY_BLOCK), lds_bytes(num_vars), s, d_sigmas,
                       num_vars, log_n, d_table, d_multi, d_ctr);
}

}  // namespace bj

extern "C" {

int bj_sigma_cells(bj_ctx *ctx, const uint64_t *d_sigmas, size_t sig_stride, unsigned num_vars, unsigned log_n, const uint64_t *h_non_residues,
                   uint32_t *d_cells, size_t cell_stride, uint64_t *first_invalid, uint64_t *num_invalid) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_sigmas || !h_non_residues || !d_cells || !first_invalid || !num_invalid)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_sigma_cells: null pointer");
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_sigma_cells: a proof is running on this context");
    std::vector<u64> table;
    if (int rc = build_table(ctx, "bj_sigma_cells", h_non_residues, num_vars, log_n, table)) return rc;
    const size_t n = (size_t)1 << log_n;
    if (sig_stride < n || cell_stride < n) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_sigma_cells: column stride below n");
    if (int rc = bj::ensure_scratch(ctx, table.size() + 2)) return rc;
    u64 *d_table = ctx->d_scratch.p, *d_ctr = d_table + table.size();
    const u64 ctr0[2] = {NONE64, 0};
    if (int rc = bj::h2d_async(ctx, d_table, table.data(), table.size() * 8)) return rc;
    if (int rc = bj::h2d_async(ctx, d_ctr, ctr0, sizeof(ctr0))) return rc;
    bj::launch_sigma_cells(d_sigmas, sig_stride, num_vars, log_n, d_table, d_cells, cell_stride, d_ctr, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    u64 ctr[2];
    if (int rc = bj_memcpy_d2h(ctx, ctr, d_ctr, sizeof(ctr))) return rc;   // synchronises
    *first_invalid = ctr[0];
    *num_invalid = ctr[1];
    return BJ_OK;
}

int bj_check_copy_constraints(bj_ctx *ctx, const bj_setup *S, const uint64_t *d_variables, bj_copy_report *out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!S || !d_variables || !out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_copy_constraints: null argument");
    if (S->device != ctx->device)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_copy_constraints: the setup lives on device %d, the context on %d", S->device, ctx->device);
    if (ctx->in_proof) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_check_copy_constraints: a proof is running on this context");
    const unsigned V = S->V, log_n = S->log_n;
    std::vector<u64> table;
    if (int rc = build_table(ctx, "bj_check_copy_constraints", S->non_residues.data(), V, log_n, table)) return rc;
    std::memset(out, 0, sizeof(*out));
    out->variable = 0xFFFFFFFFu;
    const size_t n = (size_t)1 << log_n, cells = (size_t)V << log_n;
    const size_t bitmap_words = (cells + 63) / 64;   // u64 words of one bit per cell
    const size_t o_ctr = (table.size() + 1) & ~(size_t)1, o_seen = o_ctr + 8, o_multi = o_seen + bitmap_words;
    if (int rc = bj::ensure_scratch(ctx, o_multi + bitmap_words)) return rc;
    u64 *W = ctx->d_scratch.p, *d_ctr = W + o_ctr;
    uint32_t *d_seen = (uint32_t *)(W + o_seen), *d_multi = (uint32_t *)(W + o_multi);
    hipStream_t st = ctx->stream;
    const u64 ctr0[8] = {NONE64, 0, NONE64, 0, NONE64, 0, 0, 0};
    if (int rc = bj::h2d_async(ctx, W, table.data(), table.size() * 8)) return rc;
    if (int rc = bj::h2d_async(ctx, d_ctr, ctr0, sizeof(ctr0))) return rc;
    BJ_HIP(ctx, hipMemsetAsync(d_seen, 0, 2 * bitmap_words * 8, st));
    const u64 *d_sigmas = S->d_nat;   // columns [0, V) of the replicated natural-order columns
    bj::launch_copy_check(d_sigmas, d_variables, V, log_n, W, d_seen, d_multi, d_ctr, st);
    BJ_CHECK_LAUNCH(ctx);
    u64 c[8];
    if (int rc = bj_memcpy_d2h(ctx, c, d_ctr, sizeof(c))) return rc;   // synchronises
    out->failures[BJ_COPY_SIGMA_INVALID] = c[1];
    out->failures[BJ_COPY_SIGMA_NOT_PERMUTATION] = c[3];
    out->failures[BJ_COPY_VALUE_MISMATCH] = c[5];
    u64 key;
    if (c[1]) {
        out->kind = BJ_COPY_SIGMA_INVALID;
        key = c[0];
    } else if (c[3]) {
        out->kind = BJ_COPY_SIGMA_NOT_PERMUTATION;
        bj::launch_copy_shared_target(d_sigmas, V, log_n, W, d_multi, d_ctr, st);
        BJ_CHECK_LAUNCH(ctx);
        if (int rc = bj_memcpy_d2h(ctx, &key, d_ctr + 2, 8)) return rc;
        if (key == NONE64) return bj::fail(ctx, BJ_ERR_HIP, "bj_check_copy_constraints: internal error: a target was marked twice but no entry names one");
    } else if (c[5]) {
        out->kind = BJ_COPY_VALUE_MISMATCH;
        key = c[4];
    } else {
        return BJ_OK;
    }
    const size_t col = (size_t)(key % V), row = (size_t)(key / V);
    out->column = (uint32_t)col;
    out->row = row;
    if (out->kind == BJ_COPY_SIGMA_INVALID) return BJ_OK;
    // the cell the named cell's sigma names: one word back, decoded on the host by the kernels' own decoder
    u64 sigma = 0;
    if (int rc = bj_memcpy_d2h(ctx, &sigma, d_sigmas + col * n + row, 8)) return rc;
    const uint32_t partner = decode_cell(gl::canon(sigma), V, log_n, host_view(table, V));
    if (partner == NO_CELL) return bj::fail(ctx, BJ_ERR_HIP, "bj_check_copy_constraints: internal error: host and device decode a sigma word differently");
    out->partner_column = partner >> log_n;
    out->partner_row = partner & (uint32_t)(n - 1);
    if (out->kind != BJ_COPY_VALUE_MISMATCH) return BJ_OK;
    u64 a = 0, b = 0;
    if (int rc = bj_memcpy_d2h(ctx, &a, d_variables + col * n + row, 8)) return rc;
    if (int rc = bj_memcpy_d2h(ctx, &b, d_variables + partner, 8)) return rc;
    out->value = gl::canon(a);
    out->partner_value = gl::canon(b);
    if (S->d_placement)
        if (int rc = bj_memcpy_d2h(ctx, &out->variable, S->d_placement + col * n + row, 4)) return rc;
    return BJ_OK;
}

}  // extern "C"
