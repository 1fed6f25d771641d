// The MDS layer of Poseidon (v1) on the device, once: the tree hasher (poseidon1.hip) keeps its weak output, the flattened
// gate's evaluator (poseidon_gate_terms.h) canonicalises it.
#pragma once
#include "gl.h"

namespace bj {

// MDS_MATRIX_EXPS of poseidon_goldilocks_naive.rs; row `row` of the matrix is 2^EXPS[(col - row) mod 12]
constexpr unsigned P1_EXPS[12] = {0, 0, 1, 0, 3, 5, 1, 8, 12, 3, 16, 10};

// x * y + c on the 64-bit multiply-add (one VALU instruction; a shift-add chain is two, v_lshl_add_u64 shifts by at most 4);
// the power of two travels in an SGPR (VOP3 has no literal operand on gfx950).  Callers bound the sums: no carry out.
__device__ __forceinline__ gl::u64 p1_mad(gl::u32 x, gl::u32 y, gl::u64 c) {
    gl::u64 r;
    asm("v_mad_u64_u32 %[r], vcc, %[x], %[y], %[c]" : [r] "=v"(r) : [x] "v"(x), [y] "s"(y), [c] "v"(c) : "vcc");
    return r;
}

// out[row] = sum_col s[col] * 2^EXPS[(col - row) mod 12] for weak s, as a weak residue.
//   A = sum lo32(s[col]) * 2^e,  B = sum hi32(s[col]) * 2^e:  each < 2^32 * sum_k 2^EXPS[k] = 2^32 * 70967 < 2^49 (no carry)
//   value = A + B * 2^32 = A + hi32(B) * 2^64 + lo32(B) * 2^32 == A + hi32(B) * EPS + lo32(B) * 2^32   (mod p, 2^64 == EPS)
//   T = A + hi32(B) * EPS < 2^49 + 2^49 (no carry);  r = T + (lo32(B) << 32) mod 2^64, "+EPS" on its wrap — after a wrap
//   r < T < 2^50, so the correction cannot carry again.
__device__ __forceinline__ void p1_mds(gl::u64 (&s)[12]) {
    using gl::u32;
    using gl::u64;
    u64 out[12];
#pragma unroll
    for (int row = 0; row < 12; row++) {
        u64 A = 0, B = 0;
#pragma unroll
        for (int col = 0; col < 12; col++) {
            const u32 m = 1u << P1_EXPS[(col + 12 - row) % 12];
            A = p1_mad(gl::lo32(s[col]), m, A);
            B = p1_mad(gl::hi32(s[col]), m, B);
        }
        const u64 T = p1_mad(gl::hi32(B), 0xFFFFFFFFu, A);
        u32 c;
        const u32 hi = __builtin_addc(gl::hi32(T), gl::lo32(B), 0u, &c);
        out[row] = gl::pack(gl::lo32(T), hi) + (c ? 0xFFFFFFFFull : 0ull);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = out[k];
}

}  // namespace bj
