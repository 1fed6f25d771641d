// Openings: barycentric evaluation at z and the DEEP quotient accumulation, for gfx950.
//
// Must equal (as canonical residues):
//   precompute_for_barycentric_evaluation_in_extension      src/cs/implementations/utils.rs:907-1021
//   barycentric_evaluate_{base,extension}_at_extension_...  src/cs/implementations/utils.rs:1085-1242
//   quotening_operation_in_extension                        src/cs/implementations/prover.rs:2523-2706
//
// Both are "many columns x many points" contractions with F_p^2 coefficients:
//   barycentric:  out[col] = sum_i  f_col[i] * w[i]                  (reduction over the points of coset 0)
//   DEEP:         dst[I]  += ( sum_k coef_k * f_k[I]  -  C ) / (x_I - at)   (reduction over the columns)
// A column is base-field, so coef * f is two base multiplications; an F_p^2 column (c0, c1) is presented by the host
// as two base columns with coefficients (ch0, ch1) and (7*ch1, ch0) — same residues, no special case on the device.
// The sums are accumulated UNREDUCED in gl::Acc160 (gl.h): each 64x64 product is added as a 128-bit integer into a 160-bit
// accumulator (five 32-bit words, carry chain) and reduced mod p once at the end, which replaces a modular reduction + modular
// add per term (~28 VALU ops) by the four mads + five add-with-carry (~10 ops).  HBM: every column value is read once.
#include "gl.h"
#include "kernels.h"
#include "tiled_layout.h"

using gl::u64;
using gl::u32;

namespace bj {

// ---------------------------------------------------------------------------------------------------------
// barycentric weights, stored bit-reversed:  w[j] = cf * omega^i / (z - coset*omega^i),  i = bitrev(j)
// omega^i = T[j>>1] * (-1)^(j&1) with T the bit-reversed forward twiddle table of size n.
// ---------------------------------------------------------------------------------------------------------
__global__ void barycentric_weights_kernel(u64 *w0, u64 *w1, const u64 *tw, unsigned log_n, u64 coset, u64 z0, u64 z1,
                                           u64 cf0, u64 cf1) {
    size_t n = (size_t)1 << log_n;
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    u64 wi = gl::domain_point(tw, j);
    u64 x = gl::mul(coset, wi);
    // 1 / (z - x) in F_p^2: gl::e2_inv_chain with the norm's two squares taken in the other order
    u64 d0 = gl::sub(z0, x), d1 = z1;
    u64 norm = gl::sub(gl::sqr(d0), gl::mul7(gl::sqr(d1)));
    u64 ni = gl::inv_chain(norm);
    gl::e2 inv{gl::mul(d0, ni), gl::neg(gl::mul(d1, ni))};
    gl::e2 c{gl::mul(cf0, wi), gl::mul(cf1, wi)};
    gl::e2 r = gl::e2_mul(inv, c);
    w0[j] = r.c0;
    w1[j] = r.c1;
}

void launch_barycentric_weights(u64 *d_w0, u64 *d_w1, const u64 *d_tw_fwd, unsigned log_n, u64 coset, const u64 *at,
                                hipStream_t s) {
    size_t n = (size_t)1 << log_n;
    if (n == 1) {  // utils.rs:919-927
        u64 one = 1, zero = 0;
        (void)hipMemcpyAsync(d_w0, &one, 8, hipMemcpyHostToDevice, s);
        (void)hipMemcpyAsync(d_w1, &zero, 8, hipMemcpyHostToDevice, s);
        (void)hipStreamSynchronize(s);
        return;
    }
    coset = gl::canon(coset);
    gl::e2 z{gl::canon(at[0]), gl::canon(at[1])};
    // constant factor = coset * (z^n - coset^n) / (n * coset^n)
    u64 t = gl::pow(coset, n);
    gl::e2 zn{1, 0}, base = z;
    for (size_t e = n; e; e >>= 1) {
        if (e & 1) zn = gl::e2_mul(zn, base);
        base = gl::e2_sqr(base);
    }
    zn.c0 = gl::sub(zn.c0, t);
    gl::e2 cf = gl::e2_mul_base(zn, coset);
    cf = gl::e2_mul_base(cf, gl::inv(gl::mul(t, gl::canon((u64)n % gl::P))));
    unsigned tpb = 256;
    hipLaunchKernelGGL(barycentric_weights_kernel, dim3((unsigned)((n + tpb - 1) / tpb)), dim3(tpb), 0, s, d_w0, d_w1,
                       d_tw_fwd, log_n, coset, z.c0, z.c1, cf.c0, cf.c1);
}

// ---------------------------------------------------------------------------------------------------------
// barycentric evaluation of a batch of base columns:  partial[col][block] = sum over the block's points of f * w
// ---------------------------------------------------------------------------------------------------------
// BARY_PTS (callee_words.h): points per lane, a workgroup covers 256 * BARY_PTS consecutive points
static constexpr int BARY_STEP = 4;   // points in flight per column
static constexpr int BARY_COLS = 8;   // columns sharing one read of the weights

// A lane walks its BARY_PTS points four at a time and keeps one 160-bit accumulator pair per column for the whole walk: the
// weights are read once per eight columns, and the cross-lane reduction — the larger half of this kernel when it ran after
// every eight points of every column — happens once per workgroup, for all sixteen sums together, through a transposed LDS tree.
__global__ void __launch_bounds__(256)
barycentric_partial_kernel(const u64 *const *cols, unsigned n_cols, size_t n, const u64 *w0, const u64 *w1,
                           u64 *partials, unsigned n_blocks) {
    __shared__ u64 red[2 * BARY_COLS][256 + 1];
    const unsigned t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * (256 * BARY_PTS) + t;
    const unsigned c0 = blockIdx.y * BARY_COLS;
    const u64 *f[BARY_COLS];
#pragma unroll
    for (int c = 0; c < BARY_COLS; c++) f[c] = cols[c0 + c < n_cols ? c0 + c : c0];   // a short last group re-reads its first column; the surplus sums are dropped
    gl::Acc160 s0[BARY_COLS], s1[BARY_COLS];
#pragma unroll
    for (int c = 0; c < BARY_COLS; c++) {
        s0[c].clear();
        s1[c].clear();
    }
#pragma unroll 1
    for (int k0 = 0; k0 < BARY_PTS; k0 += BARY_STEP) {
        u64 a[BARY_STEP], b[BARY_STEP];
#pragma unroll
        for (int k = 0; k < BARY_STEP; k++) {   // past the end: a zero weight on a clamped (valid) index — no divergent loads
            const size_t i = base + (size_t)(k0 + k) * 256;
            const size_t ic = i < n ? i : n - 1;
            const u64 wa = w0[ic], wb = w1[ic];
            a[k] = i < n ? wa : 0;
            b[k] = i < n ? wb : 0;
        }
#pragma unroll
        for (int c = 0; c < BARY_COLS; c++) {
            u64 v[BARY_STEP];
#pragma unroll
            for (int k = 0; k < BARY_STEP; k++) {
                const size_t i = base + (size_t)(k0 + k) * 256;
                v[k] = f[c][i < n ? i : n - 1];
            }
#pragma unroll
            for (int k = 0; k < BARY_STEP; k++) {
                s0[c].fma(v[k], a[k]);
                s1[c].fma(v[k], b[k]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < BARY_COLS; c++) {
        red[2 * c][t] = s0[c].reduce();
        red[2 * c + 1][t] = s1[c].reduce();
    }
    __syncthreads();
    {   // lane t: sum j = t & 15, the sixteen lanes' values of segment t >> 4; then sixteen lanes add the segments
        const unsigned j = t & 15, seg = t >> 4;
        u64 acc = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) acc = gl::add(acc, red[j][seg * 16 + k]);
        __syncthreads();
        red[j][seg] = acc;
        __syncthreads();
        if (t < 2 * BARY_COLS && c0 + (t >> 1) < n_cols) {
            u64 tot = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) tot = gl::add(tot, red[t][k]);
            partials[((size_t)(c0 + (t >> 1)) * n_blocks + blockIdx.x) * 2 + (t & 1)] = tot;
        }
    }
}

__global__ void barycentric_final_kernel(const u64 *partials, unsigned n_blocks, u64 *out) {
    __shared__ u64 red[2][256];
    const unsigned t = threadIdx.x, c = blockIdx.x;
    u64 s0 = 0, s1 = 0;
    for (unsigned b = t; b < n_blocks; b += 256) {
        s0 = gl::add(s0, partials[((size_t)c * n_blocks + b) * 2 + 0]);
        s1 = gl::add(s1, partials[((size_t)c * n_blocks + b) * 2 + 1]);
    }
    red[0][t] = s0;
    red[1][t] = s1;
    __syncthreads();
    for (unsigned stride = 128; stride > 0; stride >>= 1) {
        if (t < stride) {
            red[0][t] = gl::add(red[0][t], red[0][t + stride]);
            red[1][t] = gl::add(red[1][t], red[1][t + stride]);
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * c] = red[0][0];
        out[2 * c + 1] = red[1][0];
    }
}

void launch_barycentric_eval(const u64 *const *d_col_ptrs, unsigned n_cols, size_t n, const u64 *d_w0, const u64 *d_w1,
                             u64 *d_partials, u64 *d_out, hipStream_t s) {
    unsigned nb = barycentric_num_blocks(n);
    hipLaunchKernelGGL(barycentric_partial_kernel, dim3(nb, (n_cols + BARY_COLS - 1) / BARY_COLS), dim3(256), 0, s,
                       d_col_ptrs, n_cols, n, d_w0, d_w1, d_partials, nb);
    hipLaunchKernelGGL(barycentric_final_kernel, dim3(n_cols), dim3(256), 0, s, d_partials, nb, d_out);
}

// ---------------------------------------------------------------------------------------------------------
// out[i] = sum_k (coef0_k + coef1_k u) * col_k[i]  over n entries — the DEEP numerator of a large opening set taken on the
// MONOMIAL forms: sum_k c_k f_k is a polynomial of degree < n, so it is combined once over n coefficients (1/lde_factor of
// the LDE-domain traffic) and extended to the FRI domain by one two-column LDE; exact arithmetic, identical values.
// ---------------------------------------------------------------------------------------------------------
// PTS points per lane, CU columns in flight.  With few points (a 2^14-row proof has 64 wavefronts of them) the kernel is one
// long chain of dependent loads — column pointer, then value — per column: the small-n variant keeps 8 columns in flight
// and one point per lane (234 -> ~40 us at 2^14); the large-n one is throughput-bound and keeps 4 points per lane.
template <int PTS, int CU>
__global__ void __launch_bounds__(256)
linear_combination_kernel(const u64 *const *cols, const u64 *coefs /*[n_cols][2]*/, unsigned n_cols, size_t n, u64 *out0,
                          u64 *out1) {
    const size_t base = (size_t)blockIdx.x * (256 * PTS) + threadIdx.x;
    gl::Acc160 s0[PTS], s1[PTS];
#pragma unroll
    for (int k = 0; k < PTS; k++) {
        s0[k].clear();
        s1[k].clear();
    }
    unsigned c = 0;
    for (; c + CU <= n_cols; c += CU) {
        const u64 *f[CU];
        u64 v[CU][PTS];
#pragma unroll
        for (int j = 0; j < CU; j++) f[j] = cols[c + j];
#pragma unroll
        for (int j = 0; j < CU; j++)
#pragma unroll
            for (int k = 0; k < PTS; k++) {
                const size_t i = base + (size_t)k * 256;
                v[j][k] = i < n ? f[j][i] : 0;
            }
#pragma unroll
        for (int j = 0; j < CU; j++) {
            const u64 a = coefs[2 * (c + j)], b = coefs[2 * (c + j) + 1];
#pragma unroll
            for (int k = 0; k < PTS; k++) {
                s0[k].fma(v[j][k], a);
                s1[k].fma(v[j][k], b);
            }
        }
    }
    for (; c < n_cols; c++) {
        const u64 *f = cols[c];
        const u64 a = coefs[2 * c], b = coefs[2 * c + 1];
#pragma unroll
        for (int k = 0; k < PTS; k++) {
            const size_t i = base + (size_t)k * 256;
            const u64 v = i < n ? f[i] : 0;
            s0[k].fma(v, a);
            s1[k].fma(v, b);
        }
    }
#pragma unroll
    for (int k = 0; k < PTS; k++) {
        const size_t i = base + (size_t)k * 256;
        if (i < n) {
            out0[i] = s0[k].reduce();
            out1[i] = s1[k].reduce();
        }
    }
}
void launch_linear_combination(const u64 *const *d_col_ptrs, const u64 *d_coefs, unsigned n_cols, size_t n, u64 *d_out0,
                               u64 *d_out1, hipStream_t s) {
    if (n <= ((size_t)1 << 18))
        hipLaunchKernelGGL((linear_combination_kernel<1, 8>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_col_ptrs,
                           d_coefs, n_cols, n, d_out0, d_out1);
    else
        hipLaunchKernelGGL((linear_combination_kernel<4, 1>), dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, d_col_ptrs,
                           d_coefs, n_cols, n, d_out0, d_out1);
}

// ---------------------------------------------------------------------------------------------------------
// DEEP:  dst[I] (+)= ( sum_k (coef0_k + coef1_k u) * f_k[I] - (C0 + C1 u) ) / (x_I - at)
// x_I = g * w_N^{bitrev(I)} = 7 * T[I>>1] * (-1)^(I&1).  A thread owns DEEP_PTS points so that one field inversion
// (Montgomery batch trick over the norms of x_I - at) serves all of them.
// ---------------------------------------------------------------------------------------------------------
static constexpr int DEEP_PTS = 4;

// One to DEEP_MAX_SETS opening sets in one pass (the prover's z, z*omega and 0): dst (+)= sum_t (sum_k coef_tk f_tk - C_t) / (x - at_t).
// One inversion serves DEEP_PTS * n_sets denominators, and the destination is written once instead of being re-read and
// re-written per set.  Phase 1 walks (set, point) forward building the prefix products of the norms,
// phase 2 walks backward: it unwinds the inverses and computes each set's numerators only then, so that one set's
// accumulators are live at a time.  Exact arithmetic: the same values as one pass per set.
struct DeepSetDev {
    const u64 *const *cols;
    const u64 *coefs;       // [n_cols][2]
    unsigned n_cols;
    u64 c0, c1, at0, at1;
};
struct DeepSetsDev {
    DeepSetDev s[DEEP_MAX_SETS];
    int n;
};
__global__ void __launch_bounds__(256)
deep_accumulate_multi_kernel(DeepSetsDev S, size_t N, size_t I0, const u64 *tw, u64 *dst0, u64 *dst1, int accumulate) {
    const size_t base = (size_t)blockIdx.x * (256 * DEEP_PTS) + threadIdx.x;
    u64 x[DEEP_PTS];
#pragma unroll
    for (int k = 0; k < DEEP_PTS; k++) {
        const size_t I = base + (size_t)k * 256;
        const size_t Ic = I0 + (I < N ? I : 0);
        x[k] = gl::mul7(gl::domain_point(tw, Ic));
    }
    u64 norm[DEEP_MAX_SETS][DEEP_PTS], pref[DEEP_MAX_SETS][DEEP_PTS];
    u64 run = 1;
#pragma unroll
    for (int t = 0; t < DEEP_MAX_SETS; t++) {
        if (t >= S.n) break;
        const u64 seven_d1sq = gl::mul7(gl::sqr(S.s[t].at1));   // (-at1)^2 = at1^2
#pragma unroll
        for (int k = 0; k < DEEP_PTS; k++) {
            const u64 d0 = gl::sub(x[k], S.s[t].at0);
            norm[t][k] = gl::sub(gl::sqr(d0), seven_d1sq);
            pref[t][k] = run;
            run = gl::mul(run, norm[t][k]);
        }
    }
    u64 inv_run = gl::inv_chain(run);
    gl::e2 acc[DEEP_PTS];
#pragma unroll
    for (int k = 0; k < DEEP_PTS; k++) {
        const size_t I = base + (size_t)k * 256;
        acc[k] = (accumulate && I < N) ? gl::e2{gl::canon(dst0[I]), gl::canon(dst1[I])} : gl::e2{0, 0};
    }
#pragma unroll
    for (int t = DEEP_MAX_SETS - 1; t >= 0; t--) {
        if (t >= S.n) continue;
        gl::Acc160 s0[DEEP_PTS], s1[DEEP_PTS];
#pragma unroll
        for (int k = 0; k < DEEP_PTS; k++) {
            s0[k].clear();
            s1[k].clear();
        }
        for (unsigned c = 0; c < S.s[t].n_cols; c++) {
            const u64 *f = S.s[t].cols[c];
            const u64 a = S.s[t].coefs[2 * c], b = S.s[t].coefs[2 * c + 1];
#pragma unroll
            for (int k = 0; k < DEEP_PTS; k++) {
                const size_t I = base + (size_t)k * 256;
                const u64 v = f[I < N ? I : 0];
                s0[k].fma(v, a);
                s1[k].fma(v, b);
            }
        }
        const u64 d1 = gl::neg(S.s[t].at1);
#pragma unroll
        for (int k = DEEP_PTS - 1; k >= 0; k--) {
            const u64 ni = gl::mul(inv_run, pref[t][k]);
            inv_run = gl::mul(inv_run, norm[t][k]);
            const u64 d0 = gl::sub(x[k], S.s[t].at0);
            const gl::e2 den{gl::mul(d0, ni), gl::neg(gl::mul(d1, ni))};
            const gl::e2 num{gl::sub(s0[k].reduce(), S.s[t].c0), gl::sub(s1[k].reduce(), S.s[t].c1)};
            acc[k] = gl::e2_add(acc[k], gl::e2_mul(num, den));
        }
    }
#pragma unroll
    for (int k = 0; k < DEEP_PTS; k++) {
        const size_t I = base + (size_t)k * 256;
        if (I < N) {
            dst0[I] = acc[k].c0;
            dst1[I] = acc[k].c1;
        }
    }
}
void launch_deep_accumulate_multi(const ColumnSet *sets, unsigned n_sets, const u64 *const *d_ptrs, const u64 *d_coefs, size_t N,
                                  size_t I0, const u64 *d_tw_fwd, u64 *d_dst0, u64 *d_dst1, int accumulate, hipStream_t s) {
    DeepSetsDev S{};
    S.n = (int)n_sets;
    for (unsigned t = 0; t < n_sets && t < (unsigned)DEEP_MAX_SETS; t++)
        S.s[t] = DeepSetDev{d_ptrs + sets[t].first_col, d_coefs + 2 * sets[t].first_col, sets[t].n_cols, sets[t].C[0], sets[t].C[1],
                            sets[t].at[0], sets[t].at[1]};
    const unsigned blocks = (unsigned)((N + 256 * DEEP_PTS - 1) / (256 * DEEP_PTS));
    hipLaunchKernelGGL(deep_accumulate_multi_kernel, dim3(blocks), dim3(256), 0, s, S, N, I0, d_tw_fwd, d_dst0, d_dst1, accumulate);
}

// ---------------------------------------------------------------------------------------------------------
// out[j][c] = sum_i mono_c[i] * x_j^i,  x_j = 7 * w^bitrev(I0 + idx[j]): the words of leaf idx[j] of an oracle whose LDE is not kept,
// from its monomial forms (a lean setup's query openings, prover.hip).  Canonical, in the [query][column] order of gather_rows.
//
// One workgroup per (query, column); the queries are the fast grid dimension, so the workgroups that stream one column run
// together and all but the first read it out of L2 / Infinity Cache.  The exponent of a coefficient is split three ways,
//     i = lane(t) + u * 2^inner_log + k * 2^outer_log,
// so that for fixed (u, k) the 256 lanes read 256 consecutive words, and a lane's sum is
//     x^lane(t) * sum_k (x^(2^outer_log))^k * sum_u mono[...] * W[u],      W[u] = (x^(2^inner_log))^u  in LDS (one broadcast read),
// the inner sum UNREDUCED in gl::Acc160 (four mads and a carry chain per coefficient, one reduction per U of them), the outer one a
// Horner step per U coefficients.  W and the lanes' own powers are built by doubling from the squares x^(2^j): log2 U + 7 products
// per lane and as many barriers, no exponentiation loop per lane.  EvalWalk is the split for a layout: the natural order, and the
// tiled one of 2^22-word columns read where it lies (tiled_layout.h), pairs (m, l & 1) across the lanes.
// ---------------------------------------------------------------------------------------------------------
static constexpr unsigned EVAL_TABLE = 2048;   // words of W: 16 KB of LDS
struct EvalWalk {
    unsigned lanes;                     // active lanes (fewer than 256 coefficients: one each)
    unsigned lane_log;                  // lane t stands for the exponent (t >> 1) * 2^lane_log + (t & 1)
    unsigned inner_log, log_U;          // inner step u < 2^log_U <= EVAL_TABLE stands for u * 2^inner_log and lies u * inner_stride words on
    unsigned outer_log, K;              // outer step k < K stands for k * 2^outer_log and lies k * outer_stride words on
    size_t inner_stride, outer_stride;
};
static EvalWalk eval_walk(unsigned log_n, bool tiled) {
    if (tiled) {
        // e = m * 4096 + 2 u + b  (u = r * 4 + (l >> 1) < 2048, b = l & 1) sits at u * 2048 + 2 m + b; 2 m + b = k * 256 + t
        static_assert(TILED_LB == 3, "eval_walk spells the tiled layout out for 8-word tiles");
        static_assert(tiled_index(0) == 0 && tiled_index(1) == 1 && tiled_index(2) == 2048 && tiled_index(8) == 4 * 2048 &&
                      tiled_index(4096) == 2 && tiled_index((size_t)1023 * 4096 + 2 * 2047 + 1) == ((size_t)1 << 22) - 1 &&
                      tiled_index((size_t)(3 * 128 + 77) * 4096 + 2 * 1234 + 1) == (size_t)1234 * 2048 + 3 * 256 + 2 * 77 + 1,
                      "eval_walk does not follow tiled_index");
        return {256, 12, 1, 11, 19, 8, 2048, 256};
    }
    if (log_n < 8) return {1u << log_n, 1, 8, 0, 8, 1, 256, 256};
    const unsigned log_U = log_n - 8 < 11 ? log_n - 8 : 11;
    return {256, 1, 8, log_U, 8 + log_U, 1u << (log_n - 8 - log_U), 256, (size_t)256 << log_U};
}
__global__ void __launch_bounds__(256)
eval_monomials_at_kernel(const u64 *mono, size_t col_stride, unsigned n_cols, EvalWalk w, const u64 *tw, size_t I0, const u64 *idx, u64 *out) {
    __shared__ u64 W[EVAL_TABLE];
    __shared__ u64 red[256];
    const unsigned t = threadIdx.x, qi = blockIdx.x, c = blockIdx.y;
    const u64 x = gl::mul7(gl::domain_point(tw, I0 + idx[qi]));
    u64 p_lane = 0, p_inner = 0, p_outer = x;   // x^(2^lane_log), x^(2^inner_log), x^(2^outer_log)
    for (unsigned j = 0; j < w.outer_log; j++) {
        if (j == w.lane_log) p_lane = p_outer;
        if (j == w.inner_log) p_inner = p_outer;
        p_outer = gl::sqr(p_outer);
    }
    // red[j] = p_lane^j, j < 128, and W[u] = p_inner^u, by doubling
    if (t == 0) red[0] = W[0] = 1;
    __syncthreads();
    u64 ps = p_lane;
    for (unsigned s = 0; s < 7; s++) {
        if (t < (1u << s)) red[t + (1u << s)] = gl::mul(red[t], ps);
        ps = gl::sqr(ps);
        __syncthreads();
    }
    ps = p_inner;
    for (unsigned s = 0; s < w.log_U; s++) {
        for (unsigned j = t; j < (1u << s); j += 256) W[j + (1u << s)] = gl::mul(W[j], ps);
        ps = gl::sqr(ps);
        __syncthreads();
    }
    const u64 lane_power = (t & 1) ? gl::mul(red[t >> 1], x) : red[t >> 1];
    __syncthreads();   // red is reused for the sums
    u64 sum = 0;
    if (t < w.lanes) {
        const unsigned U = 1u << w.log_U;
        const u64 *col = mono + (size_t)c * col_stride + t;
        for (unsigned k = w.K; k-- > 0;) {
            const u64 *p = col + (size_t)k * w.outer_stride;
            gl::Acc160 acc;
            acc.clear();
            unsigned u = 0;
            for (; u + 8 <= U; u += 8) {
                u64 v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = p[(size_t)(u + i) * w.inner_stride];
#pragma unroll
                for (int i = 0; i < 8; i++) acc.fma(v[i], W[u + i]);
            }
            for (; u < U; u++) acc.fma(p[(size_t)u * w.inner_stride], W[u]);
            sum = gl::add(gl::mul(sum, p_outer), acc.reduce());
        }
        sum = gl::mul(sum, lane_power);
    }
    red[t] = sum;
    __syncthreads();
    for (unsigned stride = 128; stride > 0; stride >>= 1) {
        if (t < stride) red[t] = gl::add(red[t], red[t + stride]);
        __syncthreads();
    }
    if (t == 0) out[(size_t)qi * n_cols + c] = red[0];
}
void launch_eval_monomials_at(const u64 *d_mono, size_t col_stride, unsigned n_cols, unsigned log_n, bool tiled, const u64 *d_tw_fwd, size_t I0,
                              const u64 *d_idx, unsigned n_idx, u64 *d_out, hipStream_t s) {
    if (!n_cols || !n_idx) return;
    hipLaunchKernelGGL(eval_monomials_at_kernel, dim3(n_idx, n_cols), dim3(256), 0, s, d_mono, col_stride, n_cols,
                       eval_walk(log_n, tiled && log_n == 22), d_tw_fwd, I0, d_idx, d_out);
}

}  // namespace bj
