// Register-radix-16 NTT pass kernels for gfx950 — the fast path of launch_ntt_passes (ntt.hip holds the generic
// fallback and the documentation of the pass decomposition).
//
// Every thread keeps 16 field elements in VGPRs and performs 4 butterfly rounds ("one radix-16 step") on them
// without touching memory; steps are separated by a transpose through LDS.  Three kernels:
//   ntt_local12_kernel   last 12 rounds on a contiguous 4096-element chunk   (3 steps, 3 LDS transposes, the last
//                        one only to make the HBM store coalesced)
//   ntt_strided8_kernel  8 rounds at stride 2^rem_log, tile = 256 x 16 elems (2 steps, 1 LDS transpose; every HBM
//                        access is a 128-byte run)
//   ntt_strided4_kernel  4 rounds at stride 2^rem_log, tile = 16 x 256 elems (1 step, no LDS)
// Twiddles: round r of group k needs T[k] * shift^(n/2^(r+1)).  The 15 twiddles (1 + 2 + 4 + 8) of a step all come from ONE value:
// with beta = T[8 kb] * sc[r + 3] (the last round's first twiddle) round s of group g needs beta^(8 >> s) * omega_16^((8 >> s) bitrev(g, s)),
// because T[2 j] is the principal square root of T[j], T[(j << s) + g] = T[j << s] * omega_(2^(s+1))^bitrev(g, s), and sc[r + 1]^2 = sc[r].
// So a step is: x[m] *= beta^m for m = 1..15 (15 generic products), then a DFT-16 whose twiddles are 16th roots of unity — signed
// powers of two (gl.h: w16), butterflies of shifts and one fold, no product: 15 of the 32 butterflies are plain sums and differences,
// 17 shift.  Per step a thread needs the 15 powers beta^1..beta^15; they are built (and coset-scaled) ONCE per workgroup and reused for
// every column the workgroup loops over: the block-uniform ones are staged in LDS, the per-thread ones stay in VGPRs.  The inverse
// transform's table holds the inverse roots: the same step with the inverse root of unity (template parameter INV).
// All LDS indices go through pad(l) = l + l/16, which makes every transpose below bank-conflict free for
// ds_read_b64 / ds_write_b64 (64 x 4-byte banks).
#include "gl.h"
#include "kernels.h"
#include "ntt_plan.h"
#include "tiled_layout.h"

#include <cstdio>
#include <cstdlib>

using gl::u64;
using gl::u32;

namespace bj {

struct R16Args {
    const u64 *in;
    u64 *out;
    const u64 *tw;           // bit-reversed twiddle table
    const u64 *round_scale;  // [n_cosets][32] or nullptr
    unsigned log_n, r0;      // r0 = first round of this pass
    unsigned n_cols, cols_per_block;
    size_t in_col_stride, in_coset_stride, out_col_stride;
};

static constexpr int R16_WAVES = 3;   // min waves per SIMD requested from the register allocator (tuned on MI355X: 2 -> 8.6 ms, 3 -> 7.9 ms, 4 -> 10.9 ms per 93 x 2^20 x 8 LDE)
static constexpr u32 TILE = 4096;
static constexpr u32 LDS_ELEMS = TILE + TILE / 16;

// The closed experiments on these passes (profiles/r05_ntt_wait_ab.txt): issuing the next column's loads ahead of
// this column's stores with LDS-only barriers, 16-byte stores out of ntt_local12, and builds without loads, stores or barriers.
// The passes are not short of latency cover — they run at the power limit — and none of it changed their wall time.

// Workgroup barrier that orders LDS traffic only: this wave's LDS operations are complete (lgkmcnt), its HBM loads and stores may
// still be in flight (__syncthreads() is a workgroup-scope fence and would drain vmcnt as well).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ u32 pad(u32 l) { return l + (l >> 4); }
__device__ __forceinline__ void set_prio(int p) {   // s_setprio takes an immediate: p is a constant after unrolling
    if (p >= 3) __builtin_amdgcn_s_setprio(3);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}
// wave-uniform base pointer + 32-bit per-lane BYTE offset: the shape the compiler turns into `global_load v, v_off, s[base]`
// (the empty asm pins the base in an SGPR pair: without it the optimiser re-associates base + offset into sixteen hoisted
// 64-bit per-lane addresses)
// A wave-uniform GLOBAL pointer the optimiser has lost track of (computed under a branch it treats as divergent): back into an
// SGPR pair, as an address-space-1 pointer — rebuilt from integers a generic pointer would turn the accesses into flat_load /
// flat_store, which count on lgkmcnt as well and would make every LDS wait a wait for HBM.
typedef const u64 __attribute__((address_space(1))) *gcptr;
typedef u64 __attribute__((address_space(1))) *gptr;
__device__ __forceinline__ gcptr uniform_gptr(const u64 *p) {
    const u64 v = reinterpret_cast<u64>(p);
    return (gcptr)gl::pack(__builtin_amdgcn_readfirstlane(gl::lo32(v)), __builtin_amdgcn_readfirstlane(gl::hi32(v)));
}
__device__ __forceinline__ u64 ld_off(gcptr base, u32 byte_off) {
    asm volatile("" : "+s"(base));
    return *(gcptr)((const char __attribute__((address_space(1))) *)base + byte_off);
}
__device__ __forceinline__ void st_off(gptr base, u32 byte_off, u64 v) {
    asm volatile("" : "+s"(base));
    *(gptr)((char __attribute__((address_space(1))) *)base + byte_off) = v;
}
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef u64x2 __attribute__((address_space(1))) *gptr2;
__device__ __forceinline__ void st_off2(gptr base, u32 byte_off, u64 v0, u64 v1) {   // byte_off a multiple of 16
    asm volatile("" : "+s"(base));
    u64x2 v;
    v.x = v0;
    v.y = v1;
    *(gptr2)((char __attribute__((address_space(1))) *)base + byte_off) = v;
}
__device__ __forceinline__ u64 ld_off(const u64 *base, u32 byte_off) {
    asm volatile("" : "+s"(base));
    return *reinterpret_cast<const u64 *>(reinterpret_cast<const char *>(base) + byte_off);
}
__device__ __forceinline__ void st_off(u64 *base, u32 byte_off, u64 v) {
    asm volatile("" : "+s"(base));
    *reinterpret_cast<u64 *>(reinterpret_cast<char *>(base) + byte_off) = v;
}

// the base of a step's powers: beta = T[8 kb] * sc[r + 3]  (r: the step's first round, kb: its group in that round)
template <bool SCALED>
__device__ __forceinline__ u64 step_base(const u64 *__restrict__ T, size_t kb, unsigned r, const u64 *__restrict__ sc) {
    u64 b = T[kb << 3];
    if (SCALED) b = gl::mul(b, sc[r + 3]);
    return b;
}
// pw[m - 1] = beta^m, m = 1..15
template <bool SCALED>
__device__ __forceinline__ void load_step_twiddles(u64 (&pw)[15], const u64 *__restrict__ T, u32 kb, unsigned r,
                                                   const u64 *__restrict__ sc) {
    pw[0] = step_base<SCALED>(T, kb, r, sc);
#pragma unroll
    for (int m = 2; m <= 15; m++) pw[m - 1] = gl::mul(pw[m / 2 - 1], pw[m - m / 2 - 1]);
}

// One radix-16 step = 4 rounds on 16 register-resident elements; round s pairs x[i], x[i + (8>>s)] inside groups of 16>>s.  The
// elements are WEAK residues (any u64) from the load of the first pass to the store of the last one: nothing is canonicalised in
// between (the last pass does it once per element when it stores).
// pw: the step's 15 powers beta^1..beta^15, in registers (array) or in LDS (pointer) — indexed by constants either way.  The step
// multiplies x[m] by beta^m (gl::mul_weak) and runs the shift-only DFT-16: round s of group g has the twiddle omega_16^((8 >> s) bitrev(g, s)),
// butterflies two at a time through gl::w16_butterfly2_weak.
// UNIT_FIRST: beta = 1 (group 0 of an unscaled transform's first rounds): no products at all.
// FIRST_S = 2 runs only the last two of the four rounds (the local pass after a front pass that has already done the other two): four
// DFT-4 with a base of their own each, pw[3 g + m - 1] = beta_g^m for m = 1..3, beta_g = T[8 kb + 2 g] * sc[r + 3].  FIRST_S = 3 runs the
// last round alone, generic butterflies on its eight twiddles pw[7 + g] = T[8 kb + g] * sc[r + 3] (nothing to factor in one round).
// PRIO: the wave lowers its issue priority round by round (3, 2, 1, 0): the SIMD's arbiter serves the oldest wave first, so the waves
// of a workgroup would reach the barrier behind the step one after the other and the last one would compute alone; with the
// priority falling as a wave advances, the wave that is behind is served first and they arrive together (ntt_front10)
template <bool UNIT_FIRST, int FIRST_S = 0, bool PRIO = false, bool INV = false>
__device__ __forceinline__ void radix16(u64 (&x)[16], const u64 *pw) {
    if constexpr (FIRST_S == 3) {
#pragma unroll
        for (int g = 0; g < 8; g += 2) gl::butterfly2_weak(x[2 * g], x[2 * g + 1], pw[7 + g], x[2 * g + 2], x[2 * g + 3], pw[8 + g]);
    } else if constexpr (FIRST_S == 2) {
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int m = 1; m < 4; m++) x[4 * g + m] = gl::mul_weak(x[4 * g + m], pw[3 * g + m - 1]);
#pragma unroll
        for (int g = 0; g < 4; g++) gl::w16_butterfly2_weak<0, 0, INV>(x[4 * g], x[4 * g + 2], x[4 * g + 1], x[4 * g + 3]);
#pragma unroll
        for (int g = 0; g < 4; g++) gl::w16_butterfly2_weak<0, 4, INV>(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]);
    } else {
        static_assert(FIRST_S == 0, "a step runs four, two or one of its rounds");
        if (PRIO) set_prio(3);
        if (!UNIT_FIRST) {
#pragma unroll
            for (int m = 1; m < 16; m++) x[m] = gl::mul_weak(x[m], pw[m - 1]);
        }
#pragma unroll
        for (int j = 0; j < 8; j += 2) gl::w16_butterfly2_weak<0, 0, INV>(x[j], x[j + 8], x[j + 1], x[j + 9]);
        if (PRIO) set_prio(2);
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            gl::w16_butterfly2_weak<0, 0, INV>(x[j], x[j + 4], x[j + 1], x[j + 5]);
            gl::w16_butterfly2_weak<4, 4, INV>(x[j + 8], x[j + 12], x[j + 9], x[j + 13]);
        }
        if (PRIO) set_prio(1);
        gl::w16_butterfly2_weak<0, 0, INV>(x[0], x[2], x[1], x[3]);
        gl::w16_butterfly2_weak<4, 4, INV>(x[4], x[6], x[5], x[7]);
        gl::w16_butterfly2_weak<2, 2, INV>(x[8], x[10], x[9], x[11]);
        gl::w16_butterfly2_weak<6, 6, INV>(x[12], x[14], x[13], x[15]);
        if (PRIO) __builtin_amdgcn_s_setprio(0);
        gl::w16_butterfly2_weak<0, 4, INV>(x[0], x[1], x[2], x[3]);      // last round: neighbours, exponents bitrev3(g), bitrev3(g + 1)
        gl::w16_butterfly2_weak<2, 6, INV>(x[4], x[5], x[6], x[7]);
        gl::w16_butterfly2_weak<1, 5, INV>(x[8], x[9], x[10], x[11]);
        gl::w16_butterfly2_weak<3, 7, INV>(x[12], x[13], x[14], x[15]);
    }
}
// Four rounds of GENERIC butterflies on the step's 15 twiddles tw[(1<<s)-1+g] = T[(kb<<s)+g], every output multiplied by s: the last round
// runs (s u + (s w) v, s u - (s w) v) — the caller passes its eight twiddles tw[7..14] already multiplied by s — so the factor costs one
// product per butterfly.  Step C of ntt_local12_pair_tiled alone: it fetches its per-lane twiddles again for every chunk of every
// column (no room for them in registers), and fifteen loads are cheaper there than one load and fourteen products for the powers.
__device__ __forceinline__ void radix16_scaled(u64 (&x)[16], const u64 *tw, u64 s) {
#pragma unroll
    for (int st = 0; st < 3; st++) {
        const int half = 8 >> st;
#pragma unroll
        for (int g = 0; g < (1 << st); g++) {
            const u64 w = tw[(1 << st) - 1 + g];
#pragma unroll
            for (int j = 0; j < half; j += 2) {
                const int iu = g * 2 * half + j, iv = iu + half;
                gl::butterfly2_weak(x[iu], x[iv], w, x[iu + 1], x[iv + 1], w);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 8; g += 2) {
        x[2 * g] = gl::mul_weak(x[2 * g], s);
        x[2 * g + 2] = gl::mul_weak(x[2 * g + 2], s);
        gl::butterfly2_weak(x[2 * g], x[2 * g + 1], tw[7 + g], x[2 * g + 2], x[2 * g + 3], tw[8 + g]);
    }
}

// block-uniform step powers: 15 lanes compute them once, everyone reads them back as LDS broadcasts
template <bool SCALED>
__device__ __forceinline__ void stage_uniform_twiddles(u64 *lds_tw, const u64 *__restrict__ T, u32 kb, unsigned r,
                                                       const u64 *__restrict__ sc) {
    const u32 t = threadIdx.x;
    if (t < 15) lds_tw[t] = gl::pow(step_base<SCALED>(T, kb, r, sc), t + 1);
}
// the powers of sixteen consecutive groups kb0 .. kb0 + 15 of one step: tab[m * 16 + i] = beta_m^(i + 1), 240 lanes
template <bool SCALED>
__device__ __forceinline__ void stage_group_twiddles(u64 *tab, const u64 *__restrict__ T, size_t kb0, unsigned r, const u64 *__restrict__ sc) {
    const u32 t = threadIdx.x;
    if (t < 240) {
        const u32 m = t / 15, i = t % 15;
        tab[m * 16 + i] = gl::pow(step_base<SCALED>(T, kb0 + m, r, sc), i + 1);
    }
}

// ---------------------------------------------------------------------------------------------------------
// ROUNDS = 12, or 10 / 9: the same kernel without the first two / three rounds of step A (a 4096-element chunk is then four /
// eight independent sub-transforms; the rounds that remain are exactly the last ROUNDS rounds, with the twiddle indices unchanged)
template <bool SCALED, int ROUNDS = 12, bool INV = false>
__global__ void __launch_bounds__(256, R16_WAVES) ntt_local12_kernel(R16Args a) {
    __shared__ u64 lds[LDS_ELEMS + 16 + 16 * 16];
    u64 *lds_tw = lds + LDS_ELEMS;
    u64 *lds_twB = lds_tw + 16;               // [t >> 4][15 (+1 pad)] twiddles of step B (shared by 16 lanes each)
    const u32 t = threadIdx.x;
    const u32 b = blockIdx.x;
    const unsigned coset = blockIdx.z;
    const unsigned r0 = a.log_n - 12;
    const size_t n = (size_t)1 << a.log_n;
    const u64 *sc = SCALED ? a.round_scale + (size_t)coset * 32 : nullptr;

    u64 twC[15];
    load_step_twiddles<SCALED>(twC, a.tw, b * 256 + t, r0 + 8, sc);
    if (ROUNDS == 12) {
        stage_uniform_twiddles<SCALED>(lds_tw, a.tw, b, r0, sc);
    } else if (ROUNDS == 10) {   // four DFT-4: lds_tw[3 g + m - 1] = (T[8 b + 2 g] * sc[r0 + 3])^m
        if (t < 12) {
            u64 v = a.tw[(size_t)b * 8 + 2 * (t / 3)];
            if (SCALED) v = gl::mul(v, sc[r0 + 3]);
            lds_tw[t] = gl::pow(v, t % 3 + 1);
        }
    } else if (t < 8) {          // the last round of step A alone: its eight twiddles
        u64 v = a.tw[(size_t)b * 8 + t];
        if (SCALED) v = gl::mul(v, sc[r0 + 3]);
        lds_tw[7 + t] = v;
    }
    stage_group_twiddles<SCALED>(lds_twB, a.tw, (size_t)b * 16, r0 + 4, sc);
    __syncthreads();

    const unsigned col0 = blockIdx.y * a.cols_per_block;
    const unsigned col1 = min(col0 + a.cols_per_block, a.n_cols);
    const u32 ta = t >> 4, tc = t & 15;
    // The first column is peeled off the loop: the register scoreboard of the compiler is merged at a loop header, and with the
    // prologue's loads (nothing behind them) on one edge and the latch's loads (sixteen stores behind them) on the other it would
    // wait for vmcnt(0) at the top of every iteration — stores included.  With the peeled copy both edges look alike.
    u64 x[16];
    auto column = [&](unsigned col) {
        const gptr dst = (gptr)uniform_gptr(a.out + (size_t)col * a.out_col_stride + (size_t)coset * n + (size_t)b * TILE);
        const gcptr src = uniform_gptr(a.in + (size_t)col * a.in_col_stride + (size_t)coset * a.in_coset_stride + (size_t)b * TILE);
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = ld_off(src + j * 256, t * 8u);
        radix16<false, 12 - ROUNDS, false, INV>(x, lds_tw);   // step A: bits 11..8 in registers, twiddles uniform (LDS broadcasts at the point of use)
#pragma unroll
        for (int j = 0; j < 16; j++) lds[pad(j * 256 + t)] = x[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = lds[pad(ta * 256 + j * 16 + tc)];
        __syncthreads();
        radix16<false, 0, false, INV>(x, lds_twB + ta * 16);   // step B: bits 7..4
#pragma unroll
        for (int j = 0; j < 16; j++) lds[pad(ta * 256 + j * 16 + tc)] = x[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = lds[pad(t * 16 + j)];
        __syncthreads();
        radix16<false, 0, false, INV>(x, twC);   // step C: bits 3..0
#pragma unroll
        for (int j = 0; j < 16; j++) lds[pad(t * 16 + j)] = gl::canon(x[j]);   // the transform's output: canonical residues
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; j++) st_off(dst + j * 256, t * 8u, lds[pad(j * 256 + t)]);
        __syncthreads();
    };
    if (col0 >= col1) return;
    column(col0);
#pragma nounroll
    for (unsigned col = col0 + 1; col < col1; col++) column(col);
}

// ---------------------------------------------------------------------------------------------------------
static constexpr int S8_WAVES = 3;   // tuned: 3 -> 7.6 ms, 4 -> 9.7 ms (spills) per 93 x 2^20 x 8 LDE
template <bool SCALED, bool UNIT_FIRST, bool INV>
__global__ void __launch_bounds__(256, S8_WAVES) ntt_strided8_kernel(R16Args a) {
    __shared__ u64 lds[LDS_ELEMS + 16 + 16 * 16];
    u64 *lds_tw = lds + LDS_ELEMS;            // 15 block-uniform twiddles of the first step
    u64 *lds_tw2 = lds_tw + 16;               // [tm][15 (+1 pad)] twiddles of the second step: all twiddles live in LDS, which
                                              // leaves the VGPRs to the 16 data elements and lets four waves share a SIMD
    const u32 t = threadIdx.x;
    const unsigned coset = blockIdx.z;
    const unsigned rem_log = a.log_n - a.r0 - 8;          // bits of "lo" (>= 4)
    const u32 tiles_per_hi = 1u << (rem_log - 4);
    const u32 hi = blockIdx.x / tiles_per_hi, lo_tile = blockIdx.x % tiles_per_hi;
    const size_t n = (size_t)1 << a.log_n;
    const u64 *sc = SCALED ? a.round_scale + (size_t)coset * 32 : nullptr;
    const u32 tm = t >> 4, tl = t & 15;

    stage_uniform_twiddles<SCALED>(lds_tw, a.tw, hi, a.r0, sc);
    stage_group_twiddles<SCALED>(lds_tw2, a.tw, (size_t)hi * 16, a.r0 + 4, sc);   // second step: groups hi * 16 + m, m < 16
    __syncthreads();

    // addressing: a wave-uniform pointer per access (SGPR pair, advanced by scalar adds) + ONE 32-bit per-lane offset for the
    // loads and one for the stores; sixteen 64-bit per-lane addresses would cost 64 VGPRs and a wave out of every SIMD
    const size_t tile_base = ((size_t)hi << (a.log_n - a.r0)) + ((size_t)lo_tile << 4);
    const u32 off_ld = ((tm << rem_log) + tl) * 8u, off_st = (((tm * 16) << rem_log) + tl) * 8u;   // bytes; a column is < 2^32 bytes
    const unsigned col0 = blockIdx.y * a.cols_per_block;
    const unsigned col1 = min(col0 + a.cols_per_block, a.n_cols);
    u64 x[16];
    auto column = [&](unsigned col) {
        const gptr dst = (gptr)uniform_gptr(a.out + (size_t)col * a.out_col_stride + (size_t)coset * n + tile_base);
        const gcptr src = uniform_gptr(a.in + (size_t)col * a.in_col_stride + (size_t)coset * a.in_coset_stride + tile_base);
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = ld_off(src + ((size_t)(j * 16) << rem_log), off_ld);
        radix16<UNIT_FIRST, 0, false, INV>(x, lds_tw);    // mid bits 7..4
#pragma unroll
        for (int j = 0; j < 16; j++) lds[pad(j * 256 + t)] = x[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = lds[pad(tm * 256 + j * 16 + tl)];
        __syncthreads();
        radix16<false, 0, false, INV>(x, lds_tw2 + tm * 16);   // mid bits 3..0
#pragma unroll
        for (int j = 0; j < 16; j++) st_off(dst + ((size_t)j << rem_log), off_st, x[j]);
    };
    if (col0 >= col1) return;
    column(col0);          // peeled (see ntt_local12_kernel): both edges into the loop carry loads with sixteen stores behind them
#pragma nounroll
    for (unsigned col = col0 + 1; col < col1; col++) column(col);
}

// ---------------------------------------------------------------------------------------------------------
template <bool SCALED, bool UNIT_FIRST, bool INV>
__global__ void __launch_bounds__(256) ntt_strided4_kernel(R16Args a) {
    __shared__ u64 lds_tw[16];
    const u32 t = threadIdx.x;
    const unsigned coset = blockIdx.z;
    const unsigned rem_log = a.log_n - a.r0 - 4;          // >= 8
    const u32 tiles_per_hi = 1u << (rem_log - 8);
    const u32 hi = blockIdx.x / tiles_per_hi, lo_tile = blockIdx.x % tiles_per_hi;
    const size_t n = (size_t)1 << a.log_n;
    const u64 *sc = SCALED ? a.round_scale + (size_t)coset * 32 : nullptr;
    stage_uniform_twiddles<SCALED>(lds_tw, a.tw, hi, a.r0, sc);
    __syncthreads();
    u64 tw1[15];
#pragma unroll
    for (int i = 0; i < 15; i++) tw1[i] = lds_tw[i];
    const size_t base = ((size_t)hi << (a.log_n - a.r0)) + ((size_t)lo_tile << 8);
    const unsigned col0 = blockIdx.y * a.cols_per_block;
    const unsigned col1 = min(col0 + a.cols_per_block, a.n_cols);
    for (unsigned col = col0; col < col1; col++) {
        const u64 *src = a.in + (size_t)col * a.in_col_stride + (size_t)coset * a.in_coset_stride + base;
        u64 *dst = a.out + (size_t)col * a.out_col_stride + (size_t)coset * n + base;
        u64 x[16];
#pragma unroll
        for (int j = 0; j < 16; j++) x[j] = ld_off(src + ((size_t)j << rem_log), t * 8u);
        radix16<UNIT_FIRST, 0, false, INV>(x, tw1);
#pragma unroll
        for (int j = 0; j < 16; j++) st_off(dst + ((size_t)j << rem_log), t * 8u, x[j]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------
// The FIRST four rounds (strides n/2 .. n/16) of a transform with 14 + 4k rounds, for every coset at once: a lane owns the 16
// elements {i + m * n/16} of two adjacent indices i (16-byte accesses, 1 KB per wave instruction), reads them ONCE and emits
// every coset from them (an LDE reads its monomials once per column, not once per coset).  The 15 twiddles T[g] * sc[r] of
// these rounds are uniform per coset and live in LDS.  No tile and no barrier in the data path.  The pass is bound by its
// 8 * (1 + cosets) * n bytes per column, so its butterflies ride on VALU slots that would idle anyway: the local pass behind
// it then runs 10 rounds instead of 12 (ntt_local12_kernel<., 10>).
// The 2 x 16 input words of a lane stay in registers across the coset loop when every coset reads the same column (206 VGPRs: two
// waves per SIMD); with a coset stride they are read per coset.
template <bool SCALED, bool INV>
__global__ void __launch_bounds__(256, 1) ntt_first4_kernel(R16Args a, unsigned n_cosets) {
    __shared__ u64 tws[64 * 16];                          // [coset][15 (+1 pad)]
    const size_t n = (size_t)1 << a.log_n, sl = n >> 4;
    for (u32 t = threadIdx.x; t < n_cosets * 15; t += blockDim.x) {
        const u32 c = t / 15, i = t % 15;
        tws[c * 16 + i] = gl::pow(step_base<SCALED>(a.tw, 0, 0, SCALED ? a.round_scale + (size_t)c * 32 : nullptr), i + 1);
    }
    __syncthreads();
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i >= sl) return;
    const u64 *src = a.in + (size_t)blockIdx.y * a.in_col_stride + i;
    u64 *dst = a.out + (size_t)blockIdx.y * a.out_col_stride + i;
    auto load = [](const u64 *p, u64 &lo, u64 &hi) {
        const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(p);
        lo = q.x;
        hi = q.y;
    };
    const bool shared_input = a.in_coset_stride == 0;
    u64 in0[16], in1[16];
    if (shared_input) {
#pragma unroll
        for (int m = 0; m < 16; m++) load(src + (size_t)m * sl, in0[m], in1[m]);
    }
    for (unsigned c = 0; c < n_cosets; c++) {
        u64 x0[16], x1[16];
        const u64 *cs = src + (size_t)c * a.in_coset_stride;
#pragma unroll
        for (int m = 0; m < 16; m++) {
            if (shared_input) {
                x0[m] = in0[m];
                x1[m] = in1[m];
            } else {
                load(cs + (size_t)m * sl, x0[m], x1[m]);
            }
        }
        const u64 *tw = tws + c * 16;
        radix16<!SCALED, 0, false, INV>(x0, tw);   // unscaled: beta = T[0] = 1, no products
        radix16<!SCALED, 0, false, INV>(x1, tw);
        u64 *o = dst + (size_t)c * n;
#pragma unroll
        for (int m = 0; m < 16; m++) *reinterpret_cast<ulonglong2 *>(o + (size_t)m * sl) = make_ulonglong2(x0[m], x1[m]);
    }
}

// The first FIVE rounds the same way, one index per lane (32 elements {i + m * n/32} in registers): round 0 pairs the two
// halves of the register file, rounds 1..4 are one radix-16 step on each half with that half's twiddles.
template <bool SCALED, bool INV>
__global__ void __launch_bounds__(256) ntt_first5_kernel(R16Args a, unsigned n_cosets) {
    __shared__ u64 tws[64 * 40];                          // [coset]: [0] round 0; [8 + 16 h + i] step powers of half h (rounds 1..4, group h)
    const size_t n = (size_t)1 << a.log_n, sl = n >> 5;
    for (u32 t = threadIdx.x; t < n_cosets * 31; t += blockDim.x) {
        const u32 c = t / 31, i = t % 31;
        const u64 *sc = SCALED ? a.round_scale + (size_t)c * 32 : nullptr;
        if (i == 0) {
            u64 v = a.tw[0];
            if (SCALED) v = gl::mul(v, sc[0]);
            tws[c * 40] = v;
        } else {
            const u32 h = (i - 1) / 15, m = (i - 1) % 15;
            tws[c * 40 + 8 + 16 * h + m] = gl::pow(step_base<SCALED>(a.tw, h, 1, sc), m + 1);
        }
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sl) return;
    const u64 *src = a.in + (size_t)blockIdx.y * a.in_col_stride + i;
    u64 *dst = a.out + (size_t)blockIdx.y * a.out_col_stride + i;
    u64 in[32];
    if (a.in_coset_stride == 0) {
#pragma unroll
        for (int m = 0; m < 32; m++) in[m] = src[(size_t)m * sl];
    }
    for (unsigned c = 0; c < n_cosets; c++) {
        u64 lo[16], hi[16];
#pragma unroll
        for (int m = 0; m < 16; m++) {
            if (a.in_coset_stride == 0) {
                lo[m] = in[m];
                hi[m] = in[m + 16];
            } else {
                lo[m] = src[(size_t)c * a.in_coset_stride + (size_t)m * sl];
                hi[m] = src[(size_t)c * a.in_coset_stride + (size_t)(m + 16) * sl];
            }
        }
        const u64 *tw = tws + c * 40;
        const u64 w0 = tw[0];
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
            if (SCALED)
                gl::butterfly2_weak(lo[j], hi[j], w0, lo[j + 1], hi[j + 1], w0);
            else
                gl::addsub2_weak(lo[j], hi[j], lo[j + 1], hi[j + 1]);      // T[0] = 1
        }
        radix16<false, 0, false, INV>(lo, tw + 8);
        radix16<false, 0, false, INV>(hi, tw + 24);
        u64 *o = dst + (size_t)c * n;
#pragma unroll
        for (int m = 0; m < 16; m++) {
            o[(size_t)m * sl] = lo[m];
            o[(size_t)(m + 16) * sl] = hi[m];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The first TEN rounds (strides n/2 .. n/1024) of a 2^22-point transform in ONE pass over every coset: with ntt_local12 behind it
// an LDE'd column makes two HBM passes (25 n words) instead of the three of first4 + strided8 + local10 (41 n), an inverse
// transform two instead of three.  Tile = 1024 "mid" indices (the ten high bits of the element index) x 8 consecutive "lo"
// indices: 8192 elements = 64 KB of LDS, 512 threads with 16 elements each, two workgroups per CU (<= 128 VGPRs: four waves per
// SIMD), every HBM access a 64-byte run (the two tiles that share a 128-byte line are given to the same XCD back to back —
// blocks b and b + 8 — so that the halves meet in that XCD's L2).  Three register steps per coset: radix-16 on mid bits 9..6,
// radix-16 on bits 5..2, radix-4 on bits 1..0 (four lo values per lane, so that a lane stores 32 contiguous bytes), with two
// transposes through LDS in between.  LDS indices are XOR-swizzled instead of padded (tools/lds_conflicts.py: every ds_read_b64 /
// ds_write_b64 below is conflict-free), which keeps the tile at exactly 64 KB.
// Twiddles: round r < 10 of group k < 2^r needs T[k] * sc_c[r]; all of them are uniform over the tiles, so they come from a
// table per coset (1023 entries, front10_table_kernel) instead of being rebuilt by every workgroup: [0, 15) step A's fifteen powers,
// [15, 255) step B's 16 x 15 powers, [255, 1023) the twiddles of rounds 8 and 9 at [2^r - 1 + k], of which step C loads three per
// lane into registers.  The inputs of a tile are read again for every coset (no room for them in 128 VGPRs): seven of the
// eight reads are L2 / Infinity-Cache hits.
struct F10Args {
    const u64 *in;
    u64 *out;
    const u64 *tw;            // [n_cosets][1024]
    unsigned log_n, n_cols, cols_per_block, n_cosets;
    size_t in_col_stride, out_col_stride;
};
// the TILED layout of a 2^22-word column, TILED_LB and tiled_index: tiled_layout.h
__global__ void front10_table_kernel(u64 *out, const u64 *__restrict__ T, const u64 *__restrict__ round_scale, unsigned n_cosets) {
    const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_cosets * 1024u) return;
    const u32 c = idx >> 10, e = idx & 1023u;
    if (e == 1023u) {
        out[idx] = 0;
        return;
    }
    const u64 *sc = round_scale ? round_scale + (size_t)c * 32 : nullptr;
    u64 v;
    if (e < 15u) {            // step A (rounds 0..3, group 0): beta^(e + 1)
        v = gl::pow(sc ? step_base<true>(T, 0, 0, sc) : step_base<false>(T, 0, 0, sc), e + 1);
    } else if (e < 255u) {    // step B (rounds 4..7, groups mh < 16): [15 + 15 mh + m - 1] = beta_mh^m
        const u32 mh = (e - 15u) / 15u, m = (e - 15u) % 15u + 1u;
        v = gl::pow(sc ? step_base<true>(T, mh, 4, sc) : step_base<false>(T, mh, 4, sc), m);
    } else {                  // step C (rounds 8, 9): the twiddles themselves, [2^r - 1 + k] = T[k] * sc[r]
        const int r = 31 - __clz(e + 1);
        v = T[e + 1 - (1u << r)];
        if (sc) v = gl::mul(v, sc[r]);
    }
    out[idx] = gl::canon(v);
}
// The B -> C index map is LINEAR over GF(2) in the bits of (lane, register): index(lane, i) = index(lane, 0) ^ index(0, i), so a lane
// keeps ONE value for it and reaches register i's slot with one v_xor by a literal (padding would need sixteen live addresses).
// It permutes the low five index bits only: the 1024 elements of a wave's region stay inside it.  LB = log2(lo values per tile).
template <int LB>
__host__ __device__ constexpr u32 f10_bc(u32 m, u32 l) {
    const u32 x = (m << LB) + l;
    return LB == 3 ? x ^ (((x >> 3) ^ (x >> 5)) & 31u) : x ^ (((x >> 2) ^ (x >> 4)) & 31u);
}
__device__ __forceinline__ u64 &f10_at(u64 *lds, u32 byte_index) { return *reinterpret_cast<u64 *>(reinterpret_cast<char *>(lds) + byte_index); }
typedef const void __attribute__((address_space(1))) *f10_gsrc;
typedef void __attribute__((address_space(3))) *f10_ldst;
// A workgroup (8 waves) owns ONE (tile, coset) and loops over columns.  The eight cosets of a tile are eight workgroups that the
// dispatcher places on ONE XCD at the same time (block b runs on XCD b % 8: b = ((window * n_cosets + coset) * 2 + half) * 8 + xcd), so the
// tile crosses the fabric once and the other seven reads hit that XCD's L2 (measured with the cosets looped INSIDE a workgroup
// instead: FETCH_SIZE = 8 x the input, the pass ran at 4 TB/s of L2-miss traffic).  Data flow of one column:
//   the tile arrives by LDS-DMA (global_load_lds_dwordx4: no destination registers), wave w fetching the eight 1-KB pieces of
//   region w = mid bits 9..7; it is requested BEFORE the previous column's eight stores, so the counted wait at the top
//   (vmcnt(8): VMEM operations retire in order) leaves those stores in flight;                                    [barrier 1]
//   step A (mid bits 9..6 in registers) reads and writes the tile in place, in the linear order the DMA left;   [barrier 2]
//   steps B (bits 5..2) and C (bits 1..0 x four lo values) of wave w touch region w only — the B -> C transpose is an exchange
//   among the lanes of ONE wave, ordered by the wave's own LDS queue, no barrier — and when wave w has read its step-C
//   registers, region w is dead: it requests the next column's pieces at once, then computes step C and stores.
// The coset's twiddle table (8 KB) is fetched once per workgroup, by LDS-DMA as well.  The butterflies run under falling issue
// priorities (radix16's PRIO).
template <bool UNIT_FIRST, int LB, bool TILED_IN = false, bool INV = false>
__global__ void __launch_bounds__(64 << LB, 4) ntt_front10_kernel(F10Args a) {
    static_assert(!TILED_IN || LB == TILED_LB, "the tiled layout is defined for one tile width");
    constexpr u32 NT = 64u << LB, TILE_E = 1024u << LB, ROWS = 128u >> LB;   // threads, elements per tile, mid rows per 1-KB DMA piece
    __shared__ u64 lds[TILE_E + 1024];      // ONE object: tile (64 / 128 KB), twiddle table of this workgroup's coset (8 KB)
    u64 *lds_tw = lds + TILE_E;
    const u32 t = threadIdx.x;
    const u32 wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63u;
    const unsigned s_log = a.log_n - 10;
    const size_t n = (size_t)1 << a.log_n;
    const u32 b = blockIdx.x;
    u32 c, tile;
    if (LB == 3) {   // tiles 2u, 2u + 1 (the halves of 128-byte lines): blocks b, b + 8 — one XCD, back to back
        const u32 xcd = b & 7u, half = (b >> 3) & 1u, window = (b >> 4) / a.n_cosets;
        c = (b >> 4) % a.n_cosets;
        tile = window * 16u + xcd * 2u + half;
    } else {
        const u32 xcd = b & 7u, window = (b >> 3) / a.n_cosets;
        c = (b >> 3) % a.n_cosets;
        tile = window * 8u + xcd;
    }
    const size_t lo0 = (size_t)tile << LB;
    // step A: lane = (ml : mid bits 5..0, l); registers = mid bits 9..6: LDS index i * NT + t (as the DMA leaves the tile)
    // step B: lane = (mh : mid bits 9..6, mll : bits 1..0, l); registers = bits 5..2
    const u32 lB = t & ((1u << LB) - 1u), mllB = (t >> LB) & 3u, mhB = t >> (LB + 2);
    // step C: lane = (m92 : mid bits 9..2, lhi : lo bits above 1..0); registers = (mid bits 1..0, lo bits 1..0)
    const u32 lhiC = t & ((1u << (LB - 2)) - 1u), m92 = t >> (LB - 2);
    const u32 offC = (((m92 * 4u) << s_log) + lhiC * 4u) * 8u;
    const u32 ixB1 = (((mhB * 64u + mllB) << LB) + lB) * 8u, ixB2 = f10_bc<LB>(mhB * 64u + mllB, lB) * 8u, ixC = f10_bc<LB>(m92 * 4u, lhiC * 4u) * 8u;
    // DMA source of this lane inside a piece: piece p = mid rows [ROWS p, ROWS (p + 1)), lane = (row, lo pair)
    // (tiled input: the lane's 16 bytes are the words (row, l pair) at pair * 2048 + row * 2 of the tile's 1024 * 2^LB contiguous words)
    const u32 dma_off = TILED_IN ? ((lane & ((1u << (LB - 1)) - 1u)) * 2048u + (lane >> (LB - 1)) * 2u) * 8u
                                 : (((lane >> (LB - 1)) << s_log) + (lane & ((1u << (LB - 1)) - 1u)) * 2u) * 8u;
    const unsigned col0 = blockIdx.y * a.cols_per_block;
    const unsigned col1 = min(col0 + a.cols_per_block, a.n_cols);
    if (col0 >= col1) return;
    auto request_tile = [&](unsigned col) {
        const char __attribute__((address_space(1))) *src =
            (const char __attribute__((address_space(1))) *)uniform_gptr(a.in + (size_t)col * a.in_col_stride + (TILED_IN ? (size_t)tile * TILE_E : lo0)) + dma_off;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const u32 piece = wave * 8u + k;
            const size_t piece_off = TILED_IN ? (size_t)piece * ROWS * 16u : (((size_t)piece * ROWS) << s_log) * 8u;
            __builtin_amdgcn_global_load_lds((f10_gsrc)(src + piece_off), (f10_ldst)(lds + piece * 128u), 16, 0, 0);
        }
    };
    if (wave < 8u) {
        const char __attribute__((address_space(1))) *tsrc =
            (const char __attribute__((address_space(1))) *)uniform_gptr(a.tw + (size_t)c * 1024u + wave * 128u) + lane * 16u;
        __builtin_amdgcn_global_load_lds((f10_gsrc)tsrc, (f10_ldst)(lds_tw + wave * 128u), 16, 0, 0);
    }
    request_tile(col0);
    const gptr dst0 = (gptr)uniform_gptr(a.out + (size_t)c * n + lo0);
    for (unsigned col = col0; col < col1; col++) {
        // opaque copies: the sixteen xor-ed indices of an arrangement are formed where they are used, not hoisted out of the loop
        u32 jB1 = ixB1, jB2 = ixB2, jC = ixC;
        asm volatile("" : "+v"(jB1), "+v"(jB2), "+v"(jC));
        if (col == col0)
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");   // this column's pieces have landed; the last eight stores may still fly
        u64 x[16];
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = lds[i * NT + t];
        radix16<UNIT_FIRST, 0, true, INV>(x, lds_tw);
#pragma unroll
        for (int i = 0; i < 16; i++) lds[i * NT + t] = x[i];          // in place: no barrier between the read and this write
        lds_barrier();
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = f10_at(lds, jB1 + i * (32u << LB));
        radix16<false, 0, true, INV>(x, lds_tw + 15u + 15u * mhB);
#pragma unroll
        for (int i = 0; i < 16; i++) f10_at(lds, jB2 ^ (f10_bc<LB>(i * 4u, 0) * 8u)) = x[i];      // inside this wave's region
        const u64 w8 = lds_tw[255u + m92], w9a = lds_tw[511u + 2u * m92], w9b = lds_tw[512u + 2u * m92];
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = f10_at(lds, jC ^ (f10_bc<LB>(i >> 2, i & 3) * 8u));     // written by lanes of this wave
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of its region are complete: the region is dead
        if (col + 1 < col1) request_tile(col + 1);
        // round 8: mid bit 1 (registers 8 apart), group m92; round 9: mid bit 0 (registers 4 apart), groups 2 m92, 2 m92 + 1
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ll = 0; ll < 4; ll += 2) {
            gl::butterfly2_weak(x[ll], x[8 + ll], w8, x[4 + ll], x[12 + ll], w8);
            gl::butterfly2_weak(x[ll + 1], x[9 + ll], w8, x[5 + ll], x[13 + ll], w8);
        }
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int ll = 0; ll < 4; ll++) gl::butterfly2_weak(x[ll], x[4 + ll], w9a, x[8 + ll], x[12 + ll], w9b);
        const gptr dst = dst0 + (size_t)col * a.out_col_stride;
#pragma unroll
        for (int mm = 0; mm < 4; mm++) {
            st_off2(dst + ((size_t)mm << s_log), offC, x[4 * mm], x[4 * mm + 1]);
            st_off2(dst + ((size_t)mm << s_log), offC + 16u, x[4 * mm + 2], x[4 * mm + 3]);
        }
    }
}


// ---------------------------------------------------------------------------------------------------------
// LAST pass of a 2^22-point INVERSE transform whose result is kept in the tiled layout: the twelve local rounds of ntt_local12 on the
// chunk pair (b, b + 512) — one after the other through one LDS tile — the factor 1 / n, and the store.  After step C lane t holds
// the words p = 16 t + j of a chunk; their natural index is bitrev22(4096 b + p) = m * 4096 + r * 16 + l with
//     m = rev10(p & 1023) = rev4(j) * 64 + rev6(t & 63),   r = rev2(p >> 10) * 64 + (rev10(b) >> 4),   l = rev10(b) & 15,
// and rev10(b + 512) = rev10(b) + 1: the two chunks are the two halves of every 16-byte word (m, l pair) of the tiled layout, and
// for a fixed register j the 64 lanes of a wave cover 64 consecutive m — one wave store = 1 KB contiguous, straight from the
// registers (ntt_local12's third transpose through LDS, there only for the stores' sake, is not needed here).  Step C is free to
// choose WHICH sixteen-word group a lane takes: lane t takes group pi(t) = t with its low six bits reversed, so that m = rev4(j) * 64
// + (t & 63) and the lanes of a store are in address order (in lane order rev6 the same kilobyte leaves as 64 separate 16-byte
// writes: measured, the pass is then bound by them).  The twiddles of steps
// A and B of both chunks stay in LDS (2 x (16 + 256) words, as powers: radix16); step C's fifteen per lane are fetched again for every chunk
// of every column (L2 hits, issued with the chunk's sixteen data loads) — resident for both chunks they cost 60 VGPRs and the third wave
// of a SIMD — so step C keeps the generic butterflies on the twiddles themselves, with 1 / n in the last round's (radix16_scaled).
struct PairArgs {
    const u64 *in;
    u64 *out;
    const u64 *tw;           // bit-reversed twiddle table of the inverse root
    const u64 *tw_scaled;    // the same 2^21 entries times 1 / n (the last round's twiddles: radix16_scaled)
    u64 scale;               // 1 / n
    unsigned n_cols, cols_per_block;
    size_t in_col_stride, out_col_stride;
};
static constexpr int PAIR_WAVES = 3;
__global__ void __launch_bounds__(256, PAIR_WAVES) ntt_local12_pair_tiled_kernel(PairArgs a) {
    __shared__ u64 lds[LDS_ELEMS + 2 * 16 + 2 * 16 * 16];
    u64 *lds_twA = lds + LDS_ELEMS;           // [chunk][15 (+1)]
    u64 *lds_twB = lds_twA + 32;              // [chunk][t >> 4][15 (+1)]
    const u32 t = threadIdx.x;
    const u32 bp = blockIdx.x;                // chunks bp and bp + 512
    constexpr unsigned r0 = 10;
    (void)r0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const u32 b = bp + 512u * h;
        stage_uniform_twiddles<false>(lds_twA + h * 16, a.tw, b, 0, nullptr);
        stage_group_twiddles<false>(lds_twB + h * 256, a.tw, (size_t)b * 16, 0, nullptr);
    }
    __syncthreads();
    const unsigned col0 = blockIdx.y * a.cols_per_block;
    const unsigned col1 = min(col0 + a.cols_per_block, a.n_cols);
    const u32 ta = t >> 4, tc = t & 15;
    const u32 wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const u32 rb = gl::bitrev32(bp, 10);                      // even: bp < 512
    const u32 rl = gl::bitrev32(wave, 2) * 1024u + rb;        // the twelve bits (r, l) below m of this wave's natural indices (l & 1 = 0)
    const size_t tile_off = (size_t)(rl >> TILED_LB) * ((size_t)1024 << TILED_LB) + (size_t)((rl & ((1u << TILED_LB) - 1u)) >> 1) * 2048u;
    const u32 pi = (t & ~63u) | gl::bitrev32(t & 63u, 6);     // the group of sixteen words this lane takes in step C
    const u32 off_st = (t & 63u) * 16u;                       // bytes: word pair m = lane (+ rev4(j) * 64, a constant per store)
    for (unsigned col = col0; col < col1; col++) {
        u64 y[16];
#pragma nounroll   // ONE copy of the twelve rounds serves both chunks (unrolled, the loop body is ~50 KB of code for a 64 KB instruction cache)
        for (int h = 0; h < 2; h++) {
            const gcptr src = uniform_gptr(a.in + (size_t)col * a.in_col_stride + (size_t)(bp + 512u * h) * TILE);
            u64 x[16];
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = ld_off(src + j * 256, t * 8u);
            // step C's twiddles of this chunk: T[(kb << s) + g], kb = 256 b + t; the last round's from the scaled table
            u64 twC[15];
            {
                u32 kb = (bp + 512u * h) * 256u + pi;
                asm volatile("" : "+v"(kb));          // a fresh index per chunk and column: the loads stay inside the loop
#pragma unroll
                for (int st = 0; st < 4; st++)
#pragma unroll
                    for (int g = 0; g < (1 << st); g++) twC[(1 << st) - 1 + g] = (st == 3 ? a.tw_scaled : a.tw)[((size_t)kb << st) + g];
            }
            radix16<false, 0, false, true>(x, lds_twA + h * 16);      // the inverse root's table: INV
#pragma unroll
            for (int j = 0; j < 16; j++) lds[pad(j * 256 + t)] = x[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = lds[pad(ta * 256 + j * 16 + tc)];
            __syncthreads();
            radix16<false, 0, false, true>(x, lds_twB + h * 256 + ta * 16);
#pragma unroll
            for (int j = 0; j < 16; j++) lds[pad(ta * 256 + j * 16 + tc)] = x[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = lds[pad(pi * 16 + j)];
            __syncthreads();
            radix16_scaled(x, twC, a.scale);
            if (h == 0) {
#pragma unroll
                for (int j = 0; j < 16; j++) y[j] = gl::canon(x[j]);
            } else {
                const gptr dst = (gptr)uniform_gptr(a.out + (size_t)col * a.out_col_stride + tile_off);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    constexpr u32 R4[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};
                    st_off2(dst + (size_t)R4[j] * 128u, off_st, y[j], gl::canon(x[j]));
                }
            }
        }
    }
}

// natural <-> tiled re-layout of 2^22-word columns (the quotient's chunks, whose monomials come out of a transform of another size,
// and the operator-level entry points): block = (tile r, 64 consecutive m), 1024 words through LDS; natural side 64 runs of 128
// bytes, tiled side 8 runs of 1 KB
__global__ void __launch_bounds__(256) tiled_permute_kernel(const u64 *in, u64 *out, size_t in_col_stride, size_t out_col_stride, int to_tiled) {
    constexpr u32 LW = 1u << TILED_LB, PER = 64u * LW, TILE_W = 1024u * LW;   // lo values per row, words per block, words per tile
    __shared__ u64 tile[64 * (LW + 1)];
    const u32 t = threadIdx.x, r = blockIdx.x >> 4, m0 = (blockIdx.x & 15u) * 64u;
    const u64 *src = in + (size_t)blockIdx.y * in_col_stride;
    u64 *dst = out + (size_t)blockIdx.y * out_col_stride;
#pragma unroll
    for (u32 k = 0; k < PER / 256u; k++) {
        const u32 q = t + 256u * k;
        if (to_tiled) {          // natural read: q = (m local, l)
            const u32 ml = q >> TILED_LB, l = q & (LW - 1u);
            tile[ml * (LW + 1) + l] = src[((size_t)(m0 + ml) << 12) + r * LW + l];
        } else {                 // tiled read: q = (pair, m local, l & 1)
            const u32 pair = q >> 7, ml = (q >> 1) & 63u, lb = q & 1u;
            tile[ml * (LW + 1) + pair * 2 + lb] = src[(size_t)r * TILE_W + pair * 2048u + (m0 + ml) * 2u + lb];
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < PER / 256u; k++) {
        const u32 q = t + 256u * k;
        if (to_tiled) {
            const u32 pair = q >> 7, ml = (q >> 1) & 63u, lb = q & 1u;
            dst[(size_t)r * TILE_W + pair * 2048u + (m0 + ml) * 2u + lb] = tile[ml * (LW + 1) + pair * 2 + lb];
        } else {
            const u32 ml = q >> TILED_LB, l = q & (LW - 1u);
            dst[((size_t)(m0 + ml) << 12) + r * LW + l] = tile[ml * (LW + 1) + l];
        }
    }
}

// pick_cols_per_block, front10_launch_cosets, front10_cols_per_block: ntt_plan.h (tests/ntt_plan_check.cpp checks them on the host)

// which instance of a pass serves io: 0 plain forward, 1 forward on a coset (per-round scales), 2 inverse (the inverse root's table; the
// coset factors of an inverse transform are applied behind it, never as per-round scales)
static int step_mode(const NttIo &io) {
    if (io.inverse && io.round_scale) {
        fprintf(stderr, "ntt: an inverse transform takes no per-round scales\n");
        abort();
    }
    return io.inverse ? 2 : io.round_scale ? 1 : 0;
}

void launch_ntt_local12(const NttIo &io, unsigned rounds, hipStream_t s) {
    unsigned tiles = 1u << (io.log_n - 12);
    unsigned cpb = pick_cols_per_block(tiles, io.n_cols, io.n_cosets);
    // r0 = log_n - 12 whatever the round count: the kernel skips the rounds the front pass has run
    R16Args a{io.in, io.out, io.tw, io.round_scale, io.log_n, io.log_n - 12, io.n_cols, cpb, io.in_col_stride, io.in_coset_stride, io.out_col_stride};
    dim3 grid(tiles, (io.n_cols + cpb - 1) / cpb, io.n_cosets);
    void (*k)(R16Args);
    switch (step_mode(io)) {
    case 1: k = rounds == 10 ? ntt_local12_kernel<true, 10, false> : rounds == 9 ? ntt_local12_kernel<true, 9, false> : ntt_local12_kernel<true, 12, false>; break;
    case 2: k = rounds == 10 ? ntt_local12_kernel<false, 10, true> : rounds == 9 ? ntt_local12_kernel<false, 9, true> : ntt_local12_kernel<false, 12, true>; break;
    default: k = rounds == 10 ? ntt_local12_kernel<false, 10, false> : rounds == 9 ? ntt_local12_kernel<false, 9, false> : ntt_local12_kernel<false, 12, false>; break;
    }
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a);
}

// last pass of a 2^22-point inverse transform into the tiled layout (in: the front pass's output, chunk b at b * 4096)
__global__ void scale_table_kernel(const u64 *in, u64 *out, size_t count, u64 s) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = gl::mul(in[i], s);
}
void launch_scale_table(const u64 *in, u64 *out, size_t count, u64 scale, hipStream_t s) {
    hipLaunchKernelGGL(scale_table_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, in, out, count, scale);
}
void launch_ntt_local12_pair_tiled(const u64 *in, u64 *out, const u64 *tw, const u64 *tw_scaled, u64 scale, unsigned n_cols,
                                   size_t in_col_stride, size_t out_col_stride, hipStream_t s) {
    unsigned cpb = 8;
    while (cpb > 1 && (size_t)512 * ((n_cols + cpb - 1) / cpb) < 2048) cpb >>= 1;
    PairArgs a{in, out, tw, tw_scaled, scale, n_cols, cpb, in_col_stride, out_col_stride};
    hipLaunchKernelGGL(ntt_local12_pair_tiled_kernel, dim3(512, (n_cols + cpb - 1) / cpb), dim3(256), 0, s, a);
}
void launch_tiled_permute(const u64 *in, u64 *out, unsigned n_cols, size_t in_col_stride, size_t out_col_stride, bool to_tiled, hipStream_t s) {
    hipLaunchKernelGGL(tiled_permute_kernel, dim3((4096u >> TILED_LB) * 16, n_cols), dim3(256), 0, s, in, out, in_col_stride, out_col_stride, to_tiled ? 1 : 0);
}

void launch_ntt_strided(const NttIo &io, unsigned r0, unsigned rounds, hipStream_t s) {
    unsigned tiles = 1u << (io.log_n - 12);
    unsigned cpb = pick_cols_per_block(tiles, io.n_cols, io.n_cosets);
    R16Args a{io.in, io.out, io.tw, io.round_scale, io.log_n, r0, io.n_cols, cpb, io.in_col_stride, io.in_coset_stride, io.out_col_stride};
    dim3 grid(tiles, (io.n_cols + cpb - 1) / cpb, io.n_cosets);
    const int mode = step_mode(io);
    const bool unit_first = mode != 1 && r0 == 0;
    void (*k8)(R16Args), (*k4)(R16Args);
    if (mode == 1) {
        k8 = ntt_strided8_kernel<true, false, false>;
        k4 = ntt_strided4_kernel<true, false, false>;
    } else if (mode == 2) {
        k8 = unit_first ? ntt_strided8_kernel<false, true, true> : ntt_strided8_kernel<false, false, true>;
        k4 = unit_first ? ntt_strided4_kernel<false, true, true> : ntt_strided4_kernel<false, false, true>;
    } else {
        k8 = unit_first ? ntt_strided8_kernel<false, true, false> : ntt_strided8_kernel<false, false, false>;
        k4 = unit_first ? ntt_strided4_kernel<false, true, false> : ntt_strided4_kernel<false, false, false>;
    }
    hipLaunchKernelGGL(rounds == 8 ? k8 : k4, grid, dim3(256), 0, s, a);
}

void launch_ntt_first4(const NttIo &io, hipStream_t s) {
    R16Args a{io.in, io.out, io.tw, io.round_scale, io.log_n, 0, io.n_cols, 1, io.in_col_stride, io.in_coset_stride, io.out_col_stride};
    const size_t sl = ((size_t)1 << io.log_n) >> 4;
    dim3 grid((unsigned)((sl / 2 + 255) / 256), io.n_cols, 1);   // two adjacent indices per lane
    const int mode = step_mode(io);
    void (*k)(R16Args, unsigned);
    if (mode == 1) k = ntt_first4_kernel<true, false>;
    else if (mode == 2) k = ntt_first4_kernel<false, true>;
    else k = ntt_first4_kernel<false, false>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a, io.n_cosets);
}

void launch_ntt_first5(const NttIo &io, hipStream_t s) {
    R16Args a{io.in, io.out, io.tw, io.round_scale, io.log_n, 0, io.n_cols, 1, io.in_col_stride, io.in_coset_stride, io.out_col_stride};
    const size_t sl = ((size_t)1 << io.log_n) >> 5;
    dim3 grid((unsigned)((sl + 255) / 256), io.n_cols, 1);
    const int mode = step_mode(io);
    void (*k)(R16Args, unsigned);
    if (mode == 1) k = ntt_first5_kernel<true, false>;
    else if (mode == 2) k = ntt_first5_kernel<false, true>;
    else k = ntt_first5_kernel<false, false>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, a, io.n_cosets);
}

void launch_ntt_front10(const NttIo &io, u64 *d_table, bool tiled_in, hipStream_t s) {
    const unsigned n_cols = io.n_cols, n_cosets = io.n_cosets;
    const int mode = step_mode(io);
    if (tiled_in && mode == 2) {
        fprintf(stderr, "ntt: the tiled layout is read by forward transforms only\n");
        abort();
    }
    hipLaunchKernelGGL(front10_table_kernel, dim3(n_cosets * 4), dim3(256), 0, s, d_table, io.tw, io.round_scale, n_cosets);
    constexpr int LBN = 4;   // natural-order input: lo values per tile = 2^LB: 3 -> 64-byte runs, 512 threads, two workgroups per CU; 4 -> full lines, 1024 threads, one
    const int lb = tiled_in ? TILED_LB : LBN;
    const unsigned tiles = 1u << (io.log_n - 10 - lb);
    const size_t n = (size_t)1 << io.log_n;
    for (unsigned c0 = 0; c0 < n_cosets; c0 += FRONT10_COSETS_PER_LAUNCH) {   // at most eight cosets per launch: a tile's workgroups are one dispatch window on one XCD
        const unsigned nc = front10_launch_cosets(n_cosets, c0);
        const unsigned cpb = front10_cols_per_block(tiles, n_cols, nc);
        F10Args a{io.in, io.out + (size_t)c0 * n, d_table + (size_t)c0 * 1024, io.log_n, n_cols, cpb, nc, io.in_col_stride, io.out_col_stride};
        dim3 grid(tiles * nc, (n_cols + cpb - 1) / cpb, 1);
        void (*k)(F10Args);
        if (tiled_in)   // the tiled layout holds monomials: forward only
            k = mode == 1 ? ntt_front10_kernel<false, TILED_LB, true, false> : ntt_front10_kernel<true, TILED_LB, true, false>;
        else
            k = mode == 1 ? ntt_front10_kernel<false, LBN, false, false> : mode == 2 ? ntt_front10_kernel<true, LBN, false, true> : ntt_front10_kernel<true, LBN, false, false>;
        hipLaunchKernelGGL(k, grid, dim3(64u << (tiled_in ? TILED_LB : LBN)), 0, s, a);
    }
}

}  // namespace bj
