// The two flattened Poseidon gates, once: Poseidon2FlattenedGate<8, 12, 4> (src/cs/gates/poseidon2.rs:165-410) and
// PoseidonFlattenedGate<8, 12, 4, PoseidonGoldilocks> (src/cs/gates/poseidon.rs:199-464).  One repetition of either spans 130
// variables — 12 inputs, 12 outputs and a fresh variable ("degree reset") for every S-box input from the second full round on —
// and pushes 118 terms: state - variable at every reset, output_i - state_i at the end.  The walks below fix where the state is
// reset, which term is pushed and in which order; the quotient kernels (gate_poseidon.hip, canonical u64 on the device) and the
// verifier (verifier.hip, F_p^2 on the host) are the same walk under two field policies, so prover and verifier cannot disagree.
// A policy F supplies the element type and, with constants always base-field scalars: add, sub, add_rc, pow7, mul_pow2,
// mul_scalar, the Poseidon (v1) MDS layer p1_mds and dot<N> (sum_k x[k] c[k]: the dense matrix and row `v` of the fused form).
// The loop structure is the device's (the host does not care): `#pragma unroll 1` on the round loops, round 26 of v1 written out
// before rounds 27-29 (a run-time "constants or not" branch inside one loop over all four took the kernel from 79 to 252
// VGPRs), `if (k == r) s[k] = v` instead of a run-time register index.
#pragma once
#include "gl.h"
#include "poseidon1_fused.inc"   // tools/gen_poseidon1_fused_constants.py
#include "poseidon1_mds.h"
#include "poseidon_rc.inc"

namespace bj {

namespace host {
inline const gl::u64 *rc_table() {
    static const gl::u64 RC[BJ_POSEIDON_NUM_RC] = BJ_POSEIDON_RC_TABLE;
    return RC;
}
}  // namespace host

// the constant tables: __constant__ memory in device code, static tables on the host
namespace {
__constant__ gl::u64 PG_RC[BJ_POSEIDON_NUM_RC] = BJ_POSEIDON_RC_TABLE;
__constant__ gl::u64 P1G_FUSED_RC[12] = BJ_P1_FUSED_RC;
__constant__ gl::u64 P1G_DENSE[144] = BJ_P1_FUSED_DENSE;
__constant__ gl::u64 P1G_SBOX_RC[22] = BJ_P1_FUSED_SBOX_RC;
__constant__ gl::u64 P1G_VS[22 * 11] = BJ_P1_FUSED_VS;
__constant__ gl::u64 P1G_W_HATS[22 * 11] = BJ_P1_FUSED_W_HATS;
}  // namespace
struct GateTables {
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __forceinline__ const gl::u64 *rc() { return PG_RC; }
    static __device__ __forceinline__ const gl::u64 *fused_rc() { return P1G_FUSED_RC; }
    static __device__ __forceinline__ const gl::u64 *dense() { return P1G_DENSE; }
    static __device__ __forceinline__ const gl::u64 *sbox_rc() { return P1G_SBOX_RC; }
    static __device__ __forceinline__ const gl::u64 *vs() { return P1G_VS; }
    static __device__ __forceinline__ const gl::u64 *w_hats() { return P1G_W_HATS; }
#else
    static const gl::u64 *rc() { return host::rc_table(); }
    static const gl::u64 *fused_rc() { static const gl::u64 T[12] = BJ_P1_FUSED_RC; return T; }
    static const gl::u64 *dense() { static const gl::u64 T[144] = BJ_P1_FUSED_DENSE; return T; }
    static const gl::u64 *sbox_rc() { static const gl::u64 T[22] = BJ_P1_FUSED_SBOX_RC; return T; }
    static const gl::u64 *vs() { static const gl::u64 T[22 * 11] = BJ_P1_FUSED_VS; return T; }
    static const gl::u64 *w_hats() { static const gl::u64 T[22 * 11] = BJ_P1_FUSED_W_HATS; return T; }
#endif
};

// the diagonal of Poseidon2's internal matrix is 2^SH[i] (the internal layer is diag + all-ones)
constexpr unsigned P2_SH[12] = {4, 14, 11, 8, 0, 5, 2, 9, 13, 6, 3, 12};

// canonical u64: the kernels' arithmetic on the device (gl::pow7, gl::mul_pow2, Acc160 dot products, the v_mad_u64_u32 MDS);
// the same functions of gl.h on the host, the MDS by shifts
struct GateU64 : GateTables {
    using elem = gl::u64;
    static __host__ __device__ __forceinline__ elem add(elem a, elem b) { return gl::add(a, b); }
    static __host__ __device__ __forceinline__ elem sub(elem a, elem b) { return gl::sub(a, b); }
    static __host__ __device__ __forceinline__ elem add_rc(elem a, gl::u64 rc) { return gl::add(a, rc); }
    static __host__ __device__ __forceinline__ elem pow7(elem a) { return gl::pow7(a); }
    static __host__ __device__ __forceinline__ elem mul_pow2(elem a, unsigned k) { return gl::mul_pow2(a, k); }
    static __host__ __device__ __forceinline__ elem mul_scalar(elem a, gl::u64 c) { return gl::mul(a, c); }
    template <int N>
    static __host__ __device__ __forceinline__ elem dot(const elem *x, const gl::u64 *c) {
        gl::Acc160 acc;
        acc.clear();
#pragma unroll
        for (int k = 0; k < N; k++) acc.fma(x[k], c[k]);
        return acc.reduce();
    }
    static __host__ __device__ __forceinline__ void p1_mds(elem (&s)[12]) {   // M[row][col] = 2^EXPS[(col - row) mod 12]
#if defined(__HIP_DEVICE_COMPILE__)
        bj::p1_mds(s);
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] = gl::canon(s[k]);
#else
        elem out[12];
        for (int row = 0; row < 12; row++) {
            out[row] = 0;
            for (int col = 0; col < 12; col++) out[row] = gl::add(out[row], gl::mul_pow2(s[col], P1_EXPS[(col + 12 - row) % 12]));
        }
        for (int k = 0; k < 12; k++) s[k] = out[k];
#endif
    }
};

// F_p^2 on the host: the verifier's arithmetic at z
struct GateE2 : GateTables {
    using elem = gl::e2;
    static elem add(elem a, elem b) { return gl::e2_add(a, b); }
    static elem sub(elem a, elem b) { return gl::e2_sub(a, b); }
    static elem add_rc(elem a, gl::u64 rc) { return {gl::add(a.c0, gl::canon(rc)), a.c1}; }
    static elem pow7(elem x) {
        const elem x2 = gl::e2_sqr(x), x3 = gl::e2_mul(x2, x), x4 = gl::e2_sqr(x2);
        return gl::e2_mul(x4, x3);
    }
    static elem mul_pow2(elem a, unsigned k) { return gl::e2_mul_base(a, (gl::u64)1 << k); }
    static elem mul_scalar(elem a, gl::u64 c) { return gl::e2_mul_base(a, gl::canon(c)); }
    template <int N>
    static elem dot(const elem *x, const gl::u64 *c) {
        elem acc{0, 0};
        for (int k = 0; k < N; k++) acc = add(acc, mul_scalar(x[k], c[k]));
        return acc;
    }
    static void p1_mds(elem (&s)[12]) {
        elem out[12];
        for (int row = 0; row < 12; row++) {
            out[row] = {0, 0};
            for (int col = 0; col < 12; col++) out[row] = add(out[row], mul_pow2(s[col], P1_EXPS[(col + 12 - row) % 12]));
        }
        for (int k = 0; k < 12; k++) s[k] = out[k];
    }
};

// Poseidon2's external layer circ(2 M4, M4, M4), M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]] (suggested_mds.rs:21-103)
template <class F>
__host__ __device__ __forceinline__ typename F::elem gate_dbl(typename F::elem a) { return F::add(a, a); }
template <class F>
__host__ __device__ __forceinline__ void m4(typename F::elem *x) {
    using E = typename F::elem;
    const E t0 = F::add(x[0], x[1]), t1 = F::add(x[2], x[3]);
    const E t2 = F::add(gate_dbl<F>(x[1]), t1), t3 = F::add(gate_dbl<F>(x[3]), t0);
    const E t4 = F::add(gate_dbl<F>(gate_dbl<F>(t1)), t3), t5 = F::add(gate_dbl<F>(gate_dbl<F>(t0)), t2);
    x[0] = F::add(t3, t5); x[1] = t5; x[2] = F::add(t2, t4); x[3] = t4;
}
template <class F>
__host__ __device__ __forceinline__ void ext_mds(typename F::elem *s) {
    m4<F>(s); m4<F>(s + 4); m4<F>(s + 8);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const typename F::elem sum = F::add(F::add(s[j], s[4 + j]), s[8 + j]);
        s[j] = F::add(s[j], sum); s[4 + j] = F::add(s[4 + j], sum); s[8 + j] = F::add(s[8 + j], sum);
    }
}

// a degree reset of the whole state: 12 terms state_i - variable, the variables become the state
template <class F, class Var, class Push>
__host__ __device__ __forceinline__ void gate_reset(typename F::elem (&s)[12], unsigned &nxt, Var &var, Push &push) {
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const typename F::elem v = var(nxt++);
        push(F::sub(s[i], v));
        s[i] = v;
    }
}

// var(k): variable k of the repetition; push(t): the 118 terms in evaluator order
template <class F, class Var, class Push>
__host__ __device__ __forceinline__ void poseidon2_flattened_terms(Var var, Push push) {
    using E = typename F::elem;
    const gl::u64 *RC = F::rc();
    unsigned nxt = 24;
    E s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = var(i);
    ext_mds<F>(s);
#pragma unroll 1
    for (int rnd = 0; rnd < 4; rnd++) {
        if (rnd) gate_reset<F>(s, nxt, var, push);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = F::pow7(F::add_rc(s[i], RC[12 * rnd + i]));
        ext_mds<F>(s);
    }
#pragma unroll 1
    for (int rnd = 0; rnd < 22; rnd++) {
        s[0] = F::add_rc(s[0], RC[12 * (4 + rnd)]);
        const E v = var(nxt++);
        push(F::sub(s[0], v));
        s[0] = F::pow7(v);
        E tot = s[0];
#pragma unroll
        for (int i = 1; i < 12; i++) tot = F::add(tot, s[i]);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = F::add(F::mul_pow2(s[i], P2_SH[i]), tot);
    }
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        gate_reset<F>(s, nxt, var, push);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = F::pow7(F::add_rc(s[i], RC[12 * (26 + k) + i]));
        ext_mds<F>(s);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) push(F::sub(var(12 + i), s[i]));
}

// The permutation is the reference's fused form (poseidon_goldilocks.rs:374-420): after the fourth S-box layer the fused
// constants and one dense 12 x 12 matrix, then 22 partial rounds of S-box + constant on word 0 and an M'' layer (one row `v`,
// one column `w_hat`), then four full rounds whose first adds no constants.
template <class F, class Var, class Push>
__host__ __device__ __forceinline__ void poseidon1_flattened_terms(Var var, Push push) {
    using E = typename F::elem;
    const gl::u64 *RC = F::rc();
    unsigned nxt = 24;
    E s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = var(i);
#pragma unroll 1
    for (int rnd = 0; rnd < 4; rnd++) {   // full rounds 0-3; the MDS of round 3 is fused with the first partial round
        if (rnd) gate_reset<F>(s, nxt, var, push);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = F::pow7(F::add_rc(s[i], RC[12 * rnd + i]));
        if (rnd != 3) F::p1_mds(s);
    }
    {
        E t[12];
#pragma unroll
        for (int i = 0; i < 12; i++) t[i] = F::add_rc(s[i], F::fused_rc()[i]);
#pragma unroll 1
        for (int r = 0; r < 12; r++) {
            const E v = F::template dot<12>(t, F::dense() + 12 * r);
#pragma unroll
            for (int k = 0; k < 12; k++)   // s[r] = v without a run-time register index
                if (k == r) s[k] = v;
        }
    }
#pragma unroll 1
    for (int rnd = 0; rnd < 22; rnd++) {
        const E v = var(nxt++);
        push(F::sub(s[0], v));
        const E s0 = F::add_rc(F::pow7(v), F::sbox_rc()[rnd]);
        s[0] = F::add(F::template dot<11>(s + 1, F::vs() + 11 * rnd), s0);
#pragma unroll
        for (int k = 1; k < 12; k++) s[k] = F::add(s[k], F::mul_scalar(s0, F::w_hats()[11 * rnd + k - 1]));
    }
    gate_reset<F>(s, nxt, var, push);   // round 26: its constants were propagated into the partial rounds
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = F::pow7(s[i]);
    F::p1_mds(s);
#pragma unroll 1
    for (int r = 27; r < 30; r++) {
        gate_reset<F>(s, nxt, var, push);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = F::pow7(F::add_rc(s[i], RC[12 * r + i]));
        F::p1_mds(s);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) push(F::sub(var(12 + i), s[i]));
}

}  // namespace bj
