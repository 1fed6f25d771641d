// The pass plan of a 2^log_n-point transform (ntt.hip: launch_ntt_passes runs it): which kernels, over which rounds.
// Plain C++: a host compiler alone builds it, and tests/ntt_plan_check.cpp checks every row of the table below without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bj {

enum class NttPassKind : uint8_t {
    Generic,      // G(r)  ntt_pass_generic: r rounds in LDS, the whole transform of a column shorter than 2^12
    FirstRound,   // R1    ntt_first_rounds: the one remainder round of 13 + 4k
    First4,       // F4    ntt_first4: 16-byte accesses
    First5,       // F5    ntt_first5
    Front10,      // F10   ntt_front10 (its TILED_IN variant when the caller's columns are in the tiled layout)
    Strided4,     // S4    ntt_strided4
    Strided8,     // S8    ntt_strided8
    Local,        // L12, L10, L9: ntt_local12 running that many rounds
};
struct NttPass {
    NttPassKind kind;
    uint8_t r0, rounds;   // rounds [r0, r0 + rounds) of the transform
};
struct NttShape {
    unsigned log_n;
    bool aligned16;   // "a": ntt_aligned16() of the caller's columns; "u": anything else
    bool two_pass;    // env().ntt_two_pass (BJ_NTT_TWO_PASS)
};
struct NttPlan {
    unsigned n_passes;
    NttPass pass[4];
};

// columns the 16-byte accesses of ntt_first4 and ntt_front10 can take: both pointers on 16-byte boundaries, even strides
inline bool ntt_aligned16(const void *in, const void *out, size_t in_col_stride, size_t out_col_stride) {
    return (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && in_col_stride % 2 == 0 && out_col_stride % 2 == 0;
}

// The first pass reads the caller's column once for every coset (coset stride 0); every later pass runs in place on the output.
// The last 12, 10 or 9 rounds run in ntt_local12, the rounds in front of it in radix-16 strided passes of 8 or 4 rounds, and
// what 12 + 4k leaves over goes to a front pass.  That pass is bound by its traffic whatever it computes, so for 14 + 4k and
// 15 + 4k rounds it takes four or five and the local pass runs ten or nine instead of twelve: the same number of passes,
// butterflies moved into idle VALU slots (2^22: 4 + 8 + 10 measured 283.5 ms per proof, 5 + 8 + 9 284.5, 2 + 8 + 12 284.7;
// 2^23: 5 + 8 + 10 560.0 against 565.4 for 3 + 8 + 12).  The plan does not depend on the number of cosets (1..64).
//
//   log_n   plan
//   0..11   G(log_n)                    one pass; log_n = 0 is the canonicalising copy
//   12      L12
//   13      R1 L12
//   14      a: F4 L10                   u: F5 L9
//   15      F5 L10
//   16      S4 L12
//   17      R1 S4 L12
//   18      a: F4 S4 L10                u: F5 S4 L9
//   19      F5 S4 L10
//   20      S8 L12
//   21      R1 S8 L12
//   22      a: F10 L12, or F4 S8 L10 with two_pass off          u: F5 S8 L9
//   23      F5 S8 L10
//   24      S8 S4 L12
//   25      R1 S8 S4 L12
//   26      a: F4 S8 S4 L10             u: F5 S8 S4 L9
//   27      F5 S8 S4 L10
//   28      S8 S8 L12
//   29      R1 S8 S8 L12
//   30      a: F4 S8 S8 L10             u: F5 S8 S8 L9
inline NttPlan ntt_plan(const NttShape &sh) {
    NttPlan p{};
    unsigned r0 = 0;
    auto push = [&](NttPassKind kind, unsigned rounds) {
        p.pass[p.n_passes++] = NttPass{kind, (uint8_t)r0, (uint8_t)rounds};
        r0 += rounds;
    };
    if (sh.log_n < 12) {
        push(NttPassKind::Generic, sh.log_n);
        return p;
    }
    const unsigned over = (sh.log_n - 12) % 4;
    unsigned local = 12;
    if (sh.log_n == 22 && sh.aligned16 && sh.two_pass) {
        push(NttPassKind::Front10, 10);
    } else if (over == 1) {
        push(NttPassKind::FirstRound, 1);
    } else if (over == 2 && sh.aligned16) {
        push(NttPassKind::First4, 4);
        local = 10;
    } else if (over == 2) {
        push(NttPassKind::First5, 5);
        local = 9;
    } else if (over == 3) {
        push(NttPassKind::First5, 5);
        local = 10;
    }
    unsigned strided = sh.log_n - r0 - local;   // 0, 4, 8, 12 or 16
    for (; strided >= 8; strided -= 8) push(NttPassKind::Strided8, 8);
    if (strided) push(NttPassKind::Strided4, 4);
    push(NttPassKind::Local, local);
    return p;
}

// the two-pass plan: the only one that reads the tiled layout, and the one whose inverse transform can store it
inline bool ntt_plan_is_two_pass(const NttShape &sh) { return ntt_plan(sh).pass[0].kind == NttPassKind::Front10; }

// Columns per workgroup of the strided and local passes (grid: tiles x ceil(n_cols / cpb) x n_cosets, tiles = 2^(log_n - 12)).
inline unsigned pick_cols_per_block(unsigned tiles, unsigned n_cols, unsigned n_cosets) {
    // amortise the per-workgroup twiddle preparation over several columns, but keep >= ~4096 workgroups in flight
    unsigned cpb = 8;
    while (cpb > 1 && (size_t)tiles * ((n_cols + cpb - 1) / cpb) * n_cosets < 4096) cpb >>= 1;
    return cpb;
}

// ntt_front10 runs at most eight cosets per launch (a tile's workgroups are one dispatch window on one XCD): the launch that starts
// at coset c0 takes front10_launch_cosets(n_cosets, c0) of them, the next one starts FRONT10_COSETS_PER_LAUNCH further on.
constexpr unsigned FRONT10_COSETS_PER_LAUNCH = 8;
inline unsigned front10_launch_cosets(unsigned n_cosets, unsigned c0) {
    return n_cosets - c0 < FRONT10_COSETS_PER_LAUNCH ? n_cosets - c0 : FRONT10_COSETS_PER_LAUNCH;
}
// columns per workgroup of one such launch (grid: tiles * nc x ceil(n_cols / cpb), tiles = 2^(12 - log2(lo values per tile)))
inline unsigned front10_cols_per_block(unsigned tiles, unsigned n_cols, unsigned nc) {
    unsigned cpb = 8;
    while (cpb > 1 && (size_t)tiles * nc * ((n_cols + cpb - 1) / cpb) < 4096) cpb >>= 1;
    return cpb;
}

}  // namespace bj
