// Copy-permutation polynomials from the variable placement, on the device: what the reference's create_permutation_polys
// (src/cs/implementations/setup.rs:419-503) computes by walking every cell of every copiable column on one thread.
//
// Must equal, as canonical residues: with the cells numbered column-major (cell = column * n + row) and the cells of one variable
// c_0 < c_1 < ... < c_{m-1},  sigma(c_i) = id(c_{i-1}) for i >= 1  and  sigma(c_0) = id(c_{m-1}),  id(col, row) = k_col * omega^row;
// a placeholder cell and the only cell of a variable keep their own id.
//
// Plan: the placement narrowed to u32 keys (0xFFFFFFFF = placeholder, which sorts behind every variable: indices end at
// 2^32 - 2), a STABLE radix sort of (key, cell number) pairs — the cells of a variable end up next to each other in walking
// order — and one scatter pass over the sorted positions: a position writes the id of the position before it into its own
// cell, the last position of a run writes its id into the run's first cell.  The run's first position is found from its last
// one by a galloping search over the sorted keys (2 log m loads for a run of m; the common runs of 2-4 cells read neighbours
// that the wave has just loaded), which saves the head-flag scan and its buffer.  Identities are computed (one twiddle load,
// one product), never loaded; the 8-byte stores land at sorted-random addresses by the nature of the permutation.
#include "ctx.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

using gl::u32;
using gl::u64;

namespace {

constexpr u64 PLACEHOLDER_BIT = 1ull << 63, LOW_U48 = (1ull << 48) - 1;
constexpr u32 NONE = bj::PLACEMENT_NONE;

// hint cells [cols][n] (bit 63 = placeholder, low 48 bits = variable index) -> u32 keys, contiguous
__global__ void __launch_bounds__(256)
placement_narrow_kernel(const u64 *hint, size_t in_stride, unsigned log_n, size_t count, u32 *out, unsigned *bad) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u64 h = hint[(i >> log_n) * in_stride + (i & (((size_t)1 << log_n) - 1))];
    u32 k = NONE;
    if (!(h & PLACEHOLDER_BIT)) {
        const u64 idx = h & LOW_U48;
        if (idx < NONE)
            k = (u32)idx;
        else
            atomicOr(bad, 1u);
    }
    out[i] = k;
}

__global__ void __launch_bounds__(256) iota_kernel(u32 *out, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (u32)i;
}

__device__ __forceinline__ u64 cell_id(const u64 *tw, const u64 *non_res, unsigned log_n, u32 cell) {
    return gl::mul(non_res[cell >> log_n], gl::omega_pow_nat(tw, log_n, cell & ((1u << log_n) - 1)));
}

__global__ void __launch_bounds__(256)
sigma_scatter_kernel(const u32 *keys, const u32 *cells, size_t count, const u64 *non_res, const u64 *tw, unsigned log_n, u64 *sigmas,
                     size_t sig_stride) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u32 k = keys[i], c = cells[i], row_mask = (1u << log_n) - 1;
    auto at = [&](u32 cell) -> u64 & { return sigmas[(size_t)(cell >> log_n) * sig_stride + (cell & row_mask)]; };
    const bool prev_same = k != NONE && i > 0 && keys[i - 1] == k;
    const bool next_same = k != NONE && i + 1 < count && keys[i + 1] == k;
    if (prev_same) at(c) = cell_id(tw, non_res, log_n, cells[i - 1]);
    if (next_same) return;              // the run's last position writes its first cell
    if (!prev_same) {                   // placeholder, or a variable placed once
        at(c) = cell_id(tw, non_res, log_n, c);
        return;
    }
    // first position of the run: keys[lo] == k throughout; gallop down, then bisect the last stride
    size_t lo = i - 1, step = 1;
    while (lo >= step && keys[lo - step] == k) {
        lo -= step;
        step *= 2;
    }
    size_t left = lo >= step ? lo - step + 1 : 0, right = lo;
    while (left < right) {
        const size_t mid = left + (right - left) / 2;
        if (keys[mid] == k)
            right = mid;
        else
            left = mid + 1;
    }
    at(cells[left]) = cell_id(tw, non_res, log_n, c);
}

inline unsigned blocks256(size_t count) { return (unsigned)((count + 255) / 256); }

}  // namespace

namespace bj {

int placement_workspace(bj_ctx *ctx, unsigned num_vars, unsigned log_n, size_t staging_elems, PlacementWorkspace *w) {
    if (num_vars == 0) return fail(ctx, BJ_ERR_INVALID_ARG, "sigmas from placement: no columns");
    if (log_n > 30) return fail(ctx, BJ_ERR_UNSUPPORTED, "sigmas from placement: log_n %u > 30 not supported", log_n);
    if (((u64)num_vars << log_n) >= ((u64)1 << 32))
        return fail(ctx, BJ_ERR_UNSUPPORTED, "sigmas from placement: %u columns of 2^%u rows: cell numbers must fit 32 bits "
                                             "(num_vars * n < 2^32)", num_vars, log_n);
    w->cells = (size_t)num_vars << log_n;
    rocprim::double_buffer<u32> k(nullptr, nullptr), v(nullptr, nullptr);
    w->sort_bytes = 0;
    BJ_HIP(ctx, rocprim::radix_sort_pairs(nullptr, w->sort_bytes, k, v, w->cells, 0, 32, ctx->stream));
    const size_t half = (w->cells + 1) / 2, sort_elems = (w->sort_bytes + 7) / 8;   // a u32 array of `cells` in u64 words
    if (int rc = ensure_scratch(ctx, 4 * half + sort_elems + num_vars + 1 + staging_elems)) return rc;
    u64 *p = ctx->d_scratch.p;
    w->keys[0] = (u32 *)p;
    w->keys[1] = (u32 *)(p + half);
    w->vals[0] = (u32 *)(p + 2 * half);
    w->vals[1] = (u32 *)(p + 3 * half);
    w->sort_tmp = p + 4 * half;
    w->non_res = w->sort_tmp + sort_elems;
    w->bad = (unsigned *)(w->non_res + num_vars);
    w->staging = w->non_res + num_vars + 1;
    BJ_HIP(ctx, hipMemsetAsync(w->bad, 0, 8, ctx->stream));
    return BJ_OK;
}

int placement_narrow(bj_ctx *ctx, const PlacementWorkspace &w, const u64 *d_hint, size_t in_stride, unsigned cols, unsigned log_n,
                     u32 *d_out) {
    const size_t count = (size_t)cols << log_n;
    hipLaunchKernelGGL(placement_narrow_kernel, dim3(blocks256(count)), dim3(256), 0, ctx->stream, d_hint, in_stride, log_n, count, d_out,
                       w.bad);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int placement_check(bj_ctx *ctx, const PlacementWorkspace &w) {
    unsigned bad = 0;
    if (int rc = bj_memcpy_d2h(ctx, &bad, w.bad, 4)) return rc;
    if (bad) return fail(ctx, BJ_ERR_UNSUPPORTED, "sigmas from placement: a cell names a variable index above 2^32 - 2");
    return BJ_OK;
}

int sigmas_from_keys(bj_ctx *ctx, const PlacementWorkspace &w, unsigned num_vars, unsigned log_n, const u64 *h_non_residues,
                     u64 *d_sigmas, size_t sig_stride) {
    if (int rc = ensure_twiddles(ctx, log_n, false)) return rc;
    if (int rc = h2d_async(ctx, w.non_res, h_non_residues, 8 * (size_t)num_vars)) return rc;
    hipLaunchKernelGGL(iota_kernel, dim3(blocks256(w.cells)), dim3(256), 0, ctx->stream, w.vals[0], w.cells);
    BJ_CHECK_LAUNCH(ctx);
    rocprim::double_buffer<u32> keys(w.keys[0], w.keys[1]), vals(w.vals[0], w.vals[1]);
    size_t bytes = w.sort_bytes;
    BJ_HIP(ctx, rocprim::radix_sort_pairs(w.sort_tmp, bytes, keys, vals, w.cells, 0, 32, ctx->stream));
    hipLaunchKernelGGL(sigma_scatter_kernel, dim3(blocks256(w.cells)), dim3(256), 0, ctx->stream, (const u32 *)keys.current(),
                       (const u32 *)vals.current(), w.cells, (const u64 *)w.non_res, (const u64 *)ctx->tw_fwd.p, log_n, d_sigmas, sig_stride);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

}  // namespace bj

extern "C" int bj_sigmas_from_placement(bj_ctx *ctx, const uint64_t *d_placement, size_t place_stride, unsigned num_vars, unsigned log_n,
                                        const uint64_t *h_non_residues, uint64_t *d_sigmas, size_t sig_stride) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_placement || !h_non_residues || !d_sigmas) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_sigmas_from_placement: null pointer");
    bj::PlacementWorkspace w;
    if (int rc = bj::placement_workspace(ctx, num_vars, log_n, 0, &w)) return rc;
    const size_t n = (size_t)1 << log_n;
    if (place_stride < n || sig_stride < n) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_sigmas_from_placement: column stride below n");
    if (int rc = bj::placement_narrow(ctx, w, d_placement, place_stride, num_vars, log_n, w.keys[0])) return rc;
    if (int rc = bj::placement_check(ctx, w)) return rc;
    return bj::sigmas_from_keys(ctx, w, num_vars, log_n, h_non_residues, d_sigmas, sig_stride);
}
