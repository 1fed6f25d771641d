// C-ABI entry points for the opening stage (barycentric evaluation at z, DEEP quotient).  Kernels: openings.hip.
#include "ctx.h"

#include <vector>

using gl::u64;

namespace {
// [first, first + count) must lie inside the LDE domain: the kernels index the twiddle table by first + i
int check_deep_range(bj_ctx *ctx, const char *who, unsigned log_n, unsigned log_lde, size_t first, size_t count) {
    const unsigned log_full = log_n + log_lde;
    if (log_n > 32 || log_lde > 32 || log_full == 0 || log_full > 32)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: bad domain", who);
    const size_t N = (size_t)1 << log_full;
    if (count == 0 || count > N || first > N - count)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "%s: range [%zu, %zu + %zu) is empty or passes the 2^%u-point domain", who, first,
                        first, count, log_full);
    return BJ_OK;
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
    bj::launch_barycentric_weights(d_w0, d_w1, ctx->tw_fwd, log_n, coset, at2, ctx->stream);
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
    return bj::deep_accumulate_range(ctx, h_src_c0, h_src_c1, n_src, h_values, h_challenges, at2, log_n, log_lde,
                                     (size_t)1 << (log_n + log_lde), 0, d_dst_c0, d_dst_c1, accumulate);
}

int bj_deep_quotient_accumulate_range(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1,
                                      size_t n_src, const uint64_t *h_values, const uint64_t *h_challenges,
                                      const uint64_t *at2, unsigned log_n, unsigned log_lde, size_t first, size_t count,
                                      uint64_t *d_dst_c0, uint64_t *d_dst_c1, int accumulate) {
    if (int rc = bj::bind(ctx)) return rc;
    if (int rc = check_deep_range(ctx, "bj_deep_quotient_accumulate_range", log_n, log_lde, first, count)) return rc;
    return bj::deep_accumulate_range(ctx, h_src_c0, h_src_c1, n_src, h_values, h_challenges, at2, log_n, log_lde, count, first,
                                     d_dst_c0, d_dst_c1, accumulate);
}

int bj_deep_quotient_accumulate_sets(bj_ctx *ctx, const bj_deep_set *sets, unsigned n_sets, unsigned log_n,
                                     unsigned log_lde, size_t first, size_t count, uint64_t *d_dst_c0,
                                     uint64_t *d_dst_c1, int accumulate) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!sets || !d_dst_c0 || !d_dst_c1)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_deep_quotient_accumulate_sets: null pointer");
    if (n_sets == 0 || n_sets > (unsigned)bj::DEEP_MAX_SETS)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_deep_quotient_accumulate_sets: %u opening sets, one call takes 1..%d", n_sets,
                        bj::DEEP_MAX_SETS);
    if (int rc = check_deep_range(ctx, "bj_deep_quotient_accumulate_sets", log_n, log_lde, first, count)) return rc;
    bj::DeepSetHost hs[bj::DEEP_MAX_SETS];
    for (unsigned t = 0; t < n_sets; t++)
        hs[t] = bj::DeepSetHost{sets[t].src_c0, sets[t].src_c1, sets[t].n_src, sets[t].values, sets[t].challenges, sets[t].at2};
    return bj::deep_accumulate_multi(ctx, hs, n_sets, log_n, log_lde, count, first, d_dst_c0, d_dst_c1, accumulate);
}

int bj_linear_combination(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1, size_t n_src,
                          const uint64_t *h_challenges, size_t n, uint64_t *d_out_c0, uint64_t *d_out_c1) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!h_src_c0 || !h_challenges || !d_out_c0 || !d_out_c1)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_linear_combination: null pointer");
    if (n_src == 0 || n_src > (1u << 20)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_linear_combination: bad source count");
    if (n == 0) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_linear_combination: n = 0");
    for (size_t k = 0; k < n_src; k++)
        if (!h_src_c0[k]) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_linear_combination: null source %zu", k);
    return bj::combine_monomials(ctx, h_src_c0, h_src_c1, n_src, h_challenges, n, d_out_c0, d_out_c1);
}

}  // extern "C"

namespace bj {
// out = sum_k ch_k * src_k over n entries (sources: base columns, or F_p^2 columns as (c0, c1) pairs) — same flattening
// of F_p^2 sources into base columns with F_p^2 coefficients as the DEEP call below
int combine_monomials(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1, size_t n_src,
                      const uint64_t *h_challenges, size_t n, uint64_t *d_out0, uint64_t *d_out1) {
    if (int rc = bj::bind(ctx)) return rc;
    std::vector<const u64 *> ptrs;
    std::vector<u64> coefs;
    for (size_t k = 0; k < n_src; k++) {
        gl::e2 ch{gl::canon(h_challenges[2 * k]), gl::canon(h_challenges[2 * k + 1])};
        ptrs.push_back(h_src_c0[k]);
        coefs.push_back(ch.c0);
        coefs.push_back(ch.c1);
        if (h_src_c1 && h_src_c1[k]) {
            ptrs.push_back(h_src_c1[k]);
            coefs.push_back(gl::mul(gl::GEN, ch.c1));
            coefs.push_back(ch.c0);
        }
    }
    const unsigned n_cols = (unsigned)ptrs.size();
    bj::TmpBuf args;   // [pointers][F_p^2 coefficients]
    if (int rc = args.alloc(ctx, bj::column_list_arg_words(n_cols))) return rc;
    const u64 **d_ptrs = (const u64 **)args.p;
    u64 *d_coefs = (u64 *)(d_ptrs + n_cols);
    if (int rc = bj::h2d_async(ctx, (void *)d_ptrs, ptrs.data(), n_cols * sizeof(u64 *))) return rc;
    if (int rc = bj::h2d_async(ctx, d_coefs, coefs.data(), coefs.size() * sizeof(u64))) return rc;
    bj::launch_linear_combination(d_ptrs, d_coefs, n_cols, n, d_out0, d_out1, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    if (!args.from_arena) BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BJ_OK;
}

// the same over the LOCAL index range [I0, I0 + N_local) of the LDE domain (a contiguous range of cosets owned by one GPU);
// source and destination pointers address the local range
int deep_accumulate_range(bj_ctx *ctx, const uint64_t *const *h_src_c0, const uint64_t *const *h_src_c1, size_t n_src,
                          const uint64_t *h_values, const uint64_t *h_challenges, const uint64_t *at2, unsigned log_n,
                          unsigned log_lde, size_t N_local, size_t I0, uint64_t *d_dst_c0, uint64_t *d_dst_c1,
                          int accumulate) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!h_src_c0 || !h_values || !h_challenges || !at2 || !d_dst_c0 || !d_dst_c1)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_deep_quotient_accumulate: null pointer");
    if (n_src == 0 || n_src > (1u << 20)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_deep_quotient_accumulate: bad source count");
    const unsigned log_full = log_n + log_lde;
    if (log_full == 0 || log_full > 32) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_deep_quotient_accumulate: bad domain");
    if (int rc = bj::ensure_twiddles(ctx, log_full, false)) return rc;
    // flatten F_p^2 sources into base columns with F_p^2 coefficients; C = sum_k ch_k * v_k
    std::vector<const u64 *> ptrs;
    std::vector<u64> coefs;
    gl::e2 C{0, 0};
    for (size_t k = 0; k < n_src; k++) {
        if (!h_src_c0[k]) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_deep_quotient_accumulate: null source %zu", k);
        gl::e2 ch{gl::canon(h_challenges[2 * k]), gl::canon(h_challenges[2 * k + 1])};
        gl::e2 v{gl::canon(h_values[2 * k]), gl::canon(h_values[2 * k + 1])};
        C = gl::e2_add(C, gl::e2_mul(ch, v));
        ptrs.push_back(h_src_c0[k]);
        coefs.push_back(ch.c0);
        coefs.push_back(ch.c1);
        if (h_src_c1 && h_src_c1[k]) {  // (f0 + f1 u) * ch = ... + f1 * (7 ch1 + ch0 u)
            ptrs.push_back(h_src_c1[k]);
            coefs.push_back(gl::mul(gl::GEN, ch.c1));
            coefs.push_back(ch.c0);
        }
    }
    const unsigned n_cols = (unsigned)ptrs.size();
    bj::TmpBuf args;   // [pointers][F_p^2 coefficients]
    if (int rc = args.alloc(ctx, bj::column_list_arg_words(n_cols))) return rc;
    const u64 **d_ptrs = (const u64 **)args.p;
    u64 *d_coefs = (u64 *)(d_ptrs + n_cols);
    if (int rc = bj::h2d_async(ctx, (void *)d_ptrs, ptrs.data(), n_cols * sizeof(u64 *))) return rc;
    if (int rc = bj::h2d_async(ctx, d_coefs, coefs.data(), coefs.size() * sizeof(u64))) return rc;
    bj::launch_deep_accumulate(d_ptrs, d_coefs, n_cols, N_local, I0, ctx->tw_fwd, C.c0, C.c1,
                               gl::canon(at2[0]), gl::canon(at2[1]), d_dst_c0, d_dst_c1, accumulate, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    if (!args.from_arena) BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a hipMalloc'ed argument block is freed on return
    return BJ_OK;
}

// up to DEEP_MAX_SETS opening sets at once (same argument meaning per set as deep_accumulate_range): one launch, one inversion
// per lane for all of them, the destination written once
int deep_accumulate_multi(bj_ctx *ctx, const DeepSetHost *sets, unsigned n_sets, unsigned log_n, unsigned log_lde, size_t N_local,
                          size_t I0, uint64_t *d_dst_c0, uint64_t *d_dst_c1, int accumulate) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!sets || n_sets == 0 || n_sets > (unsigned)DEEP_MAX_SETS || !d_dst_c0 || !d_dst_c1)
        return bj::fail(ctx, BJ_ERR_INVALID_ARG, "deep_accumulate_multi: bad arguments");
    const unsigned log_full = log_n + log_lde;
    if (log_full == 0 || log_full > 32) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "deep_accumulate_multi: bad domain");
    if (int rc = bj::ensure_twiddles(ctx, log_full, false)) return rc;
    std::vector<const u64 *> ptrs;
    std::vector<u64> coefs;
    DeepSetHostArgs a[DEEP_MAX_SETS];
    size_t first_col[DEEP_MAX_SETS];
    for (unsigned t = 0; t < n_sets; t++) {
        const DeepSetHost &S = sets[t];
        if (!S.src_c0 || !S.values || !S.challenges || !S.at2 || S.n_src == 0 || S.n_src > (1u << 20))
            return bj::fail(ctx, BJ_ERR_INVALID_ARG, "deep_accumulate_multi: bad set %u", t);
        first_col[t] = ptrs.size();
        gl::e2 C{0, 0};
        for (size_t k = 0; k < S.n_src; k++) {
            if (!S.src_c0[k]) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "deep_accumulate_multi: null source %zu of set %u", k, t);
            const gl::e2 ch{gl::canon(S.challenges[2 * k]), gl::canon(S.challenges[2 * k + 1])};
            const gl::e2 v{gl::canon(S.values[2 * k]), gl::canon(S.values[2 * k + 1])};
            C = gl::e2_add(C, gl::e2_mul(ch, v));
            ptrs.push_back(S.src_c0[k]);
            coefs.push_back(ch.c0);
            coefs.push_back(ch.c1);
            if (S.src_c1 && S.src_c1[k]) {
                ptrs.push_back(S.src_c1[k]);
                coefs.push_back(gl::mul(gl::GEN, ch.c1));
                coefs.push_back(ch.c0);
            }
        }
        a[t].n_cols = (unsigned)(ptrs.size() - first_col[t]);
        a[t].c0 = C.c0;
        a[t].c1 = C.c1;
        a[t].at0 = gl::canon(S.at2[0]);
        a[t].at1 = gl::canon(S.at2[1]);
    }
    bj::TmpBuf args;   // [pointers][F_p^2 coefficients]
    if (int rc = args.alloc(ctx, bj::column_list_arg_words(ptrs.size()))) return rc;
    const u64 **d_ptrs = (const u64 **)args.p;
    u64 *d_coefs = (u64 *)(d_ptrs + ptrs.size());
    if (int rc = bj::h2d_async(ctx, (void *)d_ptrs, ptrs.data(), ptrs.size() * sizeof(u64 *))) return rc;
    if (int rc = bj::h2d_async(ctx, d_coefs, coefs.data(), coefs.size() * sizeof(u64))) return rc;
    for (unsigned t = 0; t < n_sets; t++) {
        a[t].d_cols = d_ptrs + first_col[t];
        a[t].d_coefs = d_coefs + 2 * first_col[t];
    }
    bj::launch_deep_accumulate_multi(a, n_sets, N_local, I0, ctx->tw_fwd, d_dst_c0, d_dst_c1, accumulate, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    if (!args.from_arena) BJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BJ_OK;
}
}  // namespace bj
