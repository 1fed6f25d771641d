// C-ABI entry points for the opening stage (barycentric evaluation at z, DEEP quotient).  Kernels: openings.hip.
#include "ctx.h"

using gl::u64;

namespace {
// a caller's sources as one set of L
int add_sources(bj_ctx *ctx, const char *who, bj::ColumnList &L, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1,
                size_t n_src, const uint64_t *h_challenges, const uint64_t *h_values, const uint64_t *at2) {
    if (n_src == 0 || n_src > (1u << 20)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: bad source count", who);
    if (!L.add_set(bj::open_srcs(h_src_c0, h_src_c1, n_src).data(), n_src, h_challenges, h_values, at2))
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: null source %zu of set %zu", who, L.bad_src, L.bad_set);
    return BJ_OK;
}

// The three DEEP entry points: the caller's sets, checked, as one column list and one launch.  [first, first + count) must lie
// inside the LDE domain (the kernel indexes the twiddle table by first + i)
int deep_sets(bj_ctx *ctx, const char *who, const bj_deep_set *sets, unsigned n_sets, unsigned log_n, unsigned log_lde, size_t first,
               size_t count, uint64_t *d_dst_c0, uint64_t *d_dst_c1, int accumulate) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!sets || !d_dst_c0 || !d_dst_c1) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: null pointer", who);
    if (n_sets == 0 || n_sets > (unsigned)bj::DEEP_MAX_SETS)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: %u opening sets, one call takes 1..%d", who, n_sets, bj::DEEP_MAX_SETS);
    const unsigned log_full = log_n + log_lde;
    if (log_n > 32 || log_lde > 32 || log_full == 0 || log_full > 32) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: bad domain", who);
    const size_t N = (size_t)1 << log_full;
    if (count == 0 || count > N || first > N - count)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: range [%zu, %zu + %zu) is empty or passes the 2^%u-point domain", who, first,
                        first, count, log_full);
    bj::ColumnList L;
    for (unsigned t = 0; t < n_sets; t++) {
        const bj_deep_set &S = sets[t];
        if (!S.src_c0 || !S.values || !S.challenges || !S.at2) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: null pointer in set %u", who, t);
        if (int rc = add_sources(ctx, who, L, S.src_c0, S.src_c1, S.n_src, S.challenges, S.values, S.at2)) return rc;
    }
    return bj::deep_accumulate_multi(ctx, L, log_n, log_lde, count, first, d_dst_c0, d_dst_c1, accumulate);
}
}  // namespace

extern "C" {

int bj_barycentric_weights(bj_ctx *ctx, unsigned log_n, uint64_t coset, const uint64_t *at2, uint64_t *d_w0,
                           uint64_t *d_w1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!at2 || !d_w0 || !d_w1) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_barycentric_weights: null pointer");
    if (log_n > 30) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_barycentric_weights: log_n > 30");
    if (gl::canon(coset) == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_barycentric_weights: zero coset");
    if (int rc = bj::ensure_twiddles(ctx, log_n ? log_n : 1, false)) return rc;
    bj::launch_barycentric_weights(d_w0, d_w1, ctx->tw_fwd.p, log_n, coset, at2, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

int bj_barycentric_eval_batch(bj_ctx *ctx, const uint64_t *const *h_col_ptrs, unsigned n_cols, unsigned log_n,
                              const uint64_t *d_w0, const uint64_t *d_w1, uint64_t *h_out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (n_cols == 0) return BJ_OK;
    if (!h_col_ptrs || !d_w0 || !d_w1 || !h_out)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_barycentric_eval_batch: null pointer");
    if (log_n > 30) return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_barycentric_eval_batch: log_n > 30");
    for (unsigned c = 0; c < n_cols; c++)
        if (!h_col_ptrs[c]) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_barycentric_eval_batch: null column %u", c);
    const size_t n = (size_t)1 << log_n;
    const unsigned nb = bj::barycentric_num_blocks(n);
    bj::TmpBuf args;   // [pointers][partial sums per block][values]
    if (int rc = args.alloc(ctx, bj::barycentric_arg_words(n_cols, n))) return rc;
    const u64 **d_ptrs = (const u64 **)args.p;
    u64 *d_partials = (u64 *)(d_ptrs + n_cols);
    u64 *d_out = d_partials + (size_t)n_cols * nb * 2;
    if (int rc = bj::h2d_async(ctx, (void *)d_ptrs, h_col_ptrs, n_cols * sizeof(u64 *))) return rc;
    // barycentric, SURVEY §8d: 8 n per base column + 16 n of weights (cached across the columns of a workgroup)
    const int pb = bj::probe_begin(ctx, "barycentric_eval", 8.0 * (double)n * n_cols + 16.0 * (double)n);
    bj::launch_barycentric_eval(d_ptrs, n_cols, n, d_w0, d_w1, d_partials, d_out, ctx->stream);
    bj::probe_end(ctx, pb);
    BJ_CHECK_LAUNCH(ctx);
    return bj_memcpy_d2h(ctx, h_out, d_out, (size_t)n_cols * 2 * sizeof(u64));
}

int bj_deep_quotient_accumulate(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1,
                                size_t n_src, const uint64_t *h_values, const uint64_t *h_challenges,
                                const uint64_t *at2, unsigned log_n, unsigned log_lde, uint64_t *d_dst_c0,
                                uint64_t *d_dst_c1, int accumulate) {
    const bj_deep_set one{h_src_c0, h_src_c1, n_src, h_values, h_challenges, at2};
    const unsigned log_full = log_n + log_lde;   // the whole domain; a bad one is refused before the range is looked at
    return deep_sets(ctx, "bj_deep_quotient_accumulate", &one, 1, log_n, log_lde, 0, log_full <= 32 ? (size_t)1 << log_full : 0, d_dst_c0,
                     d_dst_c1, accumulate);
}

int bj_deep_quotient_accumulate_range(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1,
                                      size_t n_src, const uint64_t *h_values, const uint64_t *h_challenges,
                                      const uint64_t *at2, unsigned log_n, unsigned log_lde, size_t first, size_t count,
                                      uint64_t *d_dst_c0, uint64_t *d_dst_c1, int accumulate) {
    const bj_deep_set one{h_src_c0, h_src_c1, n_src, h_values, h_challenges, at2};
    return deep_sets(ctx, "bj_deep_quotient_accumulate_range", &one, 1, log_n, log_lde, first, count, d_dst_c0, d_dst_c1, accumulate);
}

int bj_deep_quotient_accumulate_sets(bj_ctx *ctx, const bj_deep_set *sets, unsigned n_sets, unsigned log_n,
                                     unsigned log_lde, size_t first, size_t count, uint64_t *d_dst_c0,
                                     uint64_t *d_dst_c1, int accumulate) {
    return deep_sets(ctx, "bj_deep_quotient_accumulate_sets", sets, n_sets, log_n, log_lde, first, count, d_dst_c0, d_dst_c1, accumulate);
}

int bj_linear_combination(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1, size_t n_src,
                          const uint64_t *h_challenges, size_t n, uint64_t *d_out_c0, uint64_t *d_out_c1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!h_src_c0 || !h_challenges || !d_out_c0 || !d_out_c1)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_linear_combination: null pointer");
    if (n == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_linear_combination: n = 0");
    bj::ColumnList L;
    if (int rc = add_sources(ctx, "bj_linear_combination", L, h_src_c0, h_src_c1, n_src, h_challenges, nullptr, nullptr)) return rc;
    return bj::combine_monomials(ctx, L, n, d_out_c0, d_out_c1);
}

int bj_eval_monomials_at(bj_ctx *ctx, const uint64_t *d_mono, size_t col_stride, unsigned n_cols, unsigned log_n, unsigned log_lde,
                         int tiled, size_t first_leaf, const uint64_t *d_idx, unsigned n_idx, uint64_t *d_out) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_mono || !d_idx || !d_out) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_eval_monomials_at: null pointer");
    const unsigned log_full = log_n + log_lde;
    if (log_n > 32 || log_lde > 32 || log_full == 0 || log_full > 32) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_eval_monomials_at: bad domain");
    if (col_stride < ((size_t)1 << log_n)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_eval_monomials_at: col_stride smaller than 2^log_n");
    if (n_cols > 65535) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_eval_monomials_at: more than 65535 columns (one grid row each)");
    if (tiled && log_n != 22)
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_eval_monomials_at: the tiled layout is defined for 2^22-word columns");
    if (first_leaf >= ((size_t)1 << log_full))   // the indices themselves are on the device: the caller's obligation
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_eval_monomials_at: first_leaf %zu passes the 2^%u-point domain", first_leaf, log_full);
    if (int rc = bj::ensure_twiddles(ctx, log_full, false)) return rc;
    bj::launch_eval_monomials_at(d_mono, col_stride, n_cols, log_n, tiled != 0, ctx->tw_fwd.p, first_leaf, d_idx, n_idx, d_out, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return BJ_OK;
}

}  // extern "C"

namespace bj {
namespace {
// The two parts of a column list in device memory: one block `args` ([pointers][coefficients], L.words() words: out of the
// proof's workspace inside a proof), filled by two copies on the context's stream
struct DeviceColumns {
    const u64 *const *ptrs;
    const u64 *coefs;
};
int upload_columns(bj_ctx *ctx, const ColumnList &L, TmpBuf &args, DeviceColumns *d) {
    if (int rc = args.alloc(ctx, L.words())) return rc;
    u64 *d_ptrs = args.p + L.ptr_offset(), *d_coefs = args.p + L.coef_offset();
    if (int rc = bj::h2d_async(ctx, d_ptrs, L.ptrs.data(), L.ptrs.size() * sizeof(u64 *))) return rc;
    if (int rc = bj::h2d_async(ctx, d_coefs, L.coefs.data(), L.coefs.size() * sizeof(u64))) return rc;
    *d = DeviceColumns{(const u64 *const *)d_ptrs, d_coefs};
    return BJ_OK;
}
// after the launch that reads the block: a hipMalloc'ed one is freed when the caller returns
int launched_on_columns(bj_ctx *ctx, const TmpBuf &args) {
    BJ_CHECK_LAUNCH(ctx);
    if (!args.from_arena) BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BJ_OK;
}
}  // namespace

// out = sum of the columns of L times their coefficients over n entries (L: one set, its values and point unused)
int combine_monomials(bj_ctx *ctx, const ColumnList &L, size_t n, uint64_t *d_out0, uint64_t *d_out1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!L.ok || L.n_cols() == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "combine_monomials: unusable column list");
    bj::TmpBuf args;
    DeviceColumns d;
    if (int rc = upload_columns(ctx, L, args, &d)) return rc;
    bj::launch_linear_combination(d.ptrs, d.coefs, (unsigned)L.n_cols(), n, d_out0, d_out1, ctx->stream);
    return launched_on_columns(ctx, args);
}

// The 1..DEEP_MAX_SETS opening sets of L over the LOCAL index range [I0, I0 + N_local) of the LDE domain (a contiguous range of
// cosets owned by one GPU; source and destination pointers address the local range): one launch, one inversion per lane for all
// of them, the destination written once
int deep_accumulate_multi(bj_ctx *ctx, const ColumnList &L, unsigned log_n, unsigned log_lde, size_t N_local, size_t I0,
                          uint64_t *d_dst_c0, uint64_t *d_dst_c1, int accumulate) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!L.ok || L.sets.empty() || L.sets.size() > (size_t)DEEP_MAX_SETS)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "deep_accumulate_multi: unusable column list");
    if (int rc = bj::ensure_twiddles(ctx, log_n + log_lde, false)) return rc;
    bj::TmpBuf args;
    DeviceColumns d;
    if (int rc = upload_columns(ctx, L, args, &d)) return rc;
    bj::launch_deep_accumulate_multi(L.sets.data(), (unsigned)L.sets.size(), d.ptrs, d.coefs, N_local, I0, ctx->tw_fwd.p, d_dst_c0, d_dst_c1,
                                     accumulate, ctx->stream);
    return launched_on_columns(ctx, args);
}
}  // namespace bj
