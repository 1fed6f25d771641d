// Internal: the TILED layout of a 2^22-word column — the monomial form between an inverse transform and whatever reads it
//  — as one index map, shared by the transforms that write and read it (ntt_r16.hip) and by the kernel that
// evaluates monomials in place (openings.hip).  Plain C++, no HIP.
#pragma once
#include <stddef.h>

namespace bj {
// element e = m * 4096 + r * 2^LB + l (m: ten bits, r: 12 - LB, l: LB = TILED_LB bits) sits at word
//     tiled(e) = r * (1024 * 2^LB) + (l >> 1) * 2048 + m * 2 + (l & 1)
// — the 1024 * 2^LB words one front-pass tile reads are contiguous, ordered so that (a) the pair of 4096-word chunks (b, b + 512) of the
// inverse transform's last pass, whose results are the words (m, l = 2k) and (m, l = 2k + 1) of FOUR tiles for every m, leaves them
// as 16-byte words in runs of 1 KB per wave store — the bit reversal of ifft_natural_to_natural (fft/mod.rs:464-491) happens in the
// store addresses, no pass of its own — and (b) the front pass fetches 16-byte words (m, l pair) for its LDS tile in [m][l] order as before.
constexpr int TILED_LB = 3;   // lo values per front-pass tile of the tiled layout = 2^LB.  3: 1024 x 8 tiles (64 KB), 512-thread workgroups, TWO per CU —
                              // their barrier phases interleave; the half-line stores of tiles 2u, 2u + 1 meet in one XCD's L2 (blocks b, b + 8).
                              // Measured with tiled (contiguous) reads: LDE 93 x 2^22 x 8 27.10 ms against 27.76 ms for 4 (full-line tiles, one
                              // 1024-thread workgroup per CU); with natural-order reads (64-byte runs) the half-line tiles had lost.
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr size_t tiled_index(size_t e) {   // e = m * 4096 + r * 2^LB + l
    return ((e & 4095u) >> TILED_LB) * ((size_t)1024 << TILED_LB) + ((e & ((1u << TILED_LB) - 1u)) >> 1) * 2048u + (e >> 12) * 2u + (e & 1u);
}
}  // namespace bj
