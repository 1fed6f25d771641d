// Hand-written evaluator of PoseidonFlattenedGate<8, 12, 4, PoseidonGoldilocks> (src/cs/gates/poseidon.rs:199-464) for the
// quotient: the Poseidon (v1) round-function gate circuits use to hash in-circuit.  One repetition spans 130 variables — 12
// inputs, 12 outputs, and a fresh variable ("degree reset") for every full S-box input from the second full round on and for
// every partial S-box input — and pushes 118 terms: state - variable at every reset, output_i - state_i at the end.  The
// permutation is the reference's fused form (poseidon_goldilocks.rs:374-420): after the fourth S-box layer the fused constants
// and one dense 12 x 12 matrix, then 22 partial rounds of S-box + constant on word 0 and an M'' layer (one row `v`, one column
// `w_hat`), then four full rounds whose first adds no constants.  Tables: poseidon1_fused.inc
// (tools/gen_poseidon1_fused_constants.py).  The op-list interpreter (gate_program.hip) runs the same gate as the 3 457
// operations on 34 slots of the capture's canonical form (3 980 recorded relations), its temporaries in scratch memory; here
// the state stays in registers and the terms go straight into the alpha-weighted gl::Acc160 accumulators.  Same terms (as
// canonical residues), same order, same proof.  Round 26 is written out before the loop over rounds 27-29: a run-time
// "constants or not" branch inside one loop over all four rounds took the kernel from 79 to 252 VGPRs.
#include "gl.h"
#include "kernels.h"
#include "poseidon1_fused.inc"
#include "poseidon_rc.inc"

using gl::u32;
using gl::u64;

namespace bj {
namespace {

__constant__ u64 P1G_RC[BJ_POSEIDON_NUM_RC] = BJ_POSEIDON_RC_TABLE;
__constant__ u64 P1G_FUSED_RC[12] = BJ_P1_FUSED_RC;
__constant__ u64 P1G_DENSE[144] = BJ_P1_FUSED_DENSE;
__constant__ u64 P1G_SBOX_RC[22] = BJ_P1_FUSED_SBOX_RC;
__constant__ u64 P1G_VS[22 * 11] = BJ_P1_FUSED_VS;
__constant__ u64 P1G_W_HATS[22 * 11] = BJ_P1_FUSED_W_HATS;

// x * y + c on the 64-bit multiply-add, the power of two in an SGPR (as poseidon1.hip); callers bound the sums: no carry out
__device__ __forceinline__ u64 p1g_mad(u32 x, u32 y, u64 c) {
    u64 r;
    asm("v_mad_u64_u32 %[r], vcc, %[x], %[y], %[c]" : [r] "=v"(r) : [x] "v"(x), [y] "s"(y), [c] "v"(c) : "vcc");
    return r;
}

// MDS_MATRIX_EXPS (poseidon_goldilocks.rs:30); M[row][col] = 2^EXPS[(col - row) mod 12]
constexpr unsigned P1G_EXPS[12] = {0, 0, 1, 0, 3, 5, 1, 8, 12, 3, 16, 10};

// s <- MDS s for canonical s, canonical out.  The 32-bit halves are summed apart (each sum < 2^32 * 70967 < 2^49) and folded
// once: value = A + B 2^32 == A + hi32(B) EPS + lo32(B) 2^32 (mod p), "+EPS" on the one possible wrap (poseidon1.hip p1_mds).
__device__ __forceinline__ void p1g_mds(u64 (&s)[12]) {
    u64 out[12];
#pragma unroll
    for (int row = 0; row < 12; row++) {
        u64 A = 0, B = 0;
#pragma unroll
        for (int col = 0; col < 12; col++) {
            const u32 m = 1u << P1G_EXPS[(col + 12 - row) % 12];
            A = p1g_mad(gl::lo32(s[col]), m, A);
            B = p1g_mad(gl::hi32(s[col]), m, B);
        }
        const u64 T = p1g_mad(gl::hi32(B), 0xFFFFFFFFu, A);
        u32 c;
        const u32 hi = __builtin_addc(gl::hi32(T), gl::lo32(B), 0u, &c);
        out[row] = gl::canon(gl::pack(gl::lo32(T), hi) + (c ? 0xFFFFFFFFull : 0ull));
    }
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = out[k];
}

__global__ void __launch_bounds__(256)
quotient_poseidon_flattened_kernel(const u64 *vars, size_t var_stride, const u64 *consts, size_t const_stride,
                                   unsigned path_len, unsigned path_bits, const u64 *alphas /* [118][2] */, size_t Q, u64 *out0,
                                   u64 *out1) {
    const size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= Q) return;
    u64 sel = 1;
    for (unsigned b = 0; b < path_len; b++) {
        u64 c = gl::canon(consts[(size_t)b * const_stride + I]);
        sel = gl::mul(sel, ((path_bits >> b) & 1u) ? c : gl::sub(1, c));
    }
    gl::Acc160 a0, a1;
    a0.clear();
    a1.clear();
    unsigned term = 0, nxt = 24;
    auto var = [&](unsigned k) { return gl::canon(vars[(size_t)k * var_stride + I]); };
    auto push = [&](u64 t) {
        a0.fma(t, alphas[2 * term]);
        a1.fma(t, alphas[2 * term + 1]);
        term++;
    };
    auto reset = [&](u64 (&s)[12]) {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const u64 v = var(nxt++);
            push(gl::sub(s[i], v));
            s[i] = v;
        }
    };
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = var(i);
#pragma unroll 1
    for (int rnd = 0; rnd < 4; rnd++) {   // full rounds 0-3; the MDS of round 3 is fused with the first partial round
        if (rnd) reset(s);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = gl::pow7(gl::add(s[i], P1G_RC[12 * rnd + i]));
        if (rnd != 3) p1g_mds(s);
    }
    {
        u64 t[12];
#pragma unroll
        for (int i = 0; i < 12; i++) t[i] = gl::add(s[i], P1G_FUSED_RC[i]);
#pragma unroll 1
        for (int r = 0; r < 12; r++) {
            gl::Acc160 acc;
            acc.clear();
#pragma unroll
            for (int k = 0; k < 12; k++) acc.fma(t[k], P1G_DENSE[12 * r + k]);
            const u64 v = acc.reduce();
#pragma unroll
            for (int k = 0; k < 12; k++)   // s[r] = v without a run-time register index
                if (k == r) s[k] = v;
        }
    }
#pragma unroll 1
    for (int rnd = 0; rnd < 22; rnd++) {
        const u64 v = var(nxt++);
        push(gl::sub(s[0], v));
        const u64 s0 = gl::add(gl::pow7(v), P1G_SBOX_RC[rnd]);
        gl::Acc160 acc;
        acc.clear();
#pragma unroll
        for (int k = 1; k < 12; k++) acc.fma(s[k], P1G_VS[11 * rnd + k - 1]);
        s[0] = gl::add(acc.reduce(), s0);
#pragma unroll
        for (int k = 1; k < 12; k++) s[k] = gl::add(s[k], gl::mul(s0, P1G_W_HATS[11 * rnd + k - 1]));
    }
    reset(s);   // round 26: its constants were propagated into the partial rounds
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl::pow7(s[i]);
    p1g_mds(s);
#pragma unroll 1
    for (int r = 27; r < 30; r++) {
        reset(s);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = gl::pow7(gl::add(s[i], P1G_RC[12 * r + i]));
        p1g_mds(s);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) push(gl::sub(var(12 + i), s[i]));
    out0[I] = gl::add(gl::canon(out0[I]), gl::mul(a0.reduce(), sel));
    out1[I] = gl::add(gl::canon(out1[I]), gl::mul(a1.reduce(), sel));
}

}  // namespace

void launch_quotient_poseidon_flattened(const u64 *d_vars, size_t var_stride, const u64 *d_consts, size_t const_stride,
                                        unsigned path_len, const unsigned char *path, const u64 *d_alphas, size_t Q,
                                        u64 *d_out0, u64 *d_out1, hipStream_t s) {
    unsigned bits = 0;
    for (unsigned b = 0; b < path_len; b++) bits |= (path[b] ? 1u : 0u) << b;
    hipLaunchKernelGGL(quotient_poseidon_flattened_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, d_vars,
                       var_stride, d_consts, const_stride, path_len, bits, d_alphas, Q, d_out0, d_out1);
}

}  // namespace bj
