#!/usr/bin/env python3
"""Generates era_boojum_amd/csrc/gl_asm.inc: hand-scheduled gfx950 instruction sequences for the lazy ("weak residue")
Goldilocks arithmetic of the NTT and Poseidon2 kernels, as inline-asm device functions.

Why a generator: the sequences write HALVES of 64-bit register pairs (v_mov into the high word of a multiply-add addend,
carry chains word by word), which compiler-allocated inline-asm operands cannot express on this target (no sub-register
operand modifier) — temporaries are therefore fixed physical VGPRs listed as clobbers; and gfx950 needs 2 wait states between
a VALU write of an SGPR pair (carry / borrow masks) and a VALU read of it, which the compiler cannot insert inside an asm
string.  The generator interleaves independent chains so that every such dependency has two other instructions in
between, checks that, and pads with s_nop only where it must.

    python tools/gen_gl_asm.py          # rewrites era_boojum_amd/csrc/gl_asm.inc (also run by era_boojum_amd/build.py)
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "era_boojum_amd", "csrc", "gl_asm.inc")

# first physical VGPR of the temporaries; low enough that kernels with ~64..80 live registers keep their occupancy
TEMP_BASE = 48


class Chain:
    """One dependent instruction sequence.  Instructions are (text, sgpr_defs, sgpr_uses)."""

    def __init__(self, name):
        self.name = name
        self.ins = []

    def add(self, text, defs=(), uses=()):
        self.ins.append((text, tuple(defs), tuple(uses)))


def pair(r):
    return "v[%d:%d]" % (r, r + 1)


def mul_chain(ch, a0, a1, b0, b1, T, X, H, Z, cm, c, bq, rare):
    """X <- weak(a * b).  T, X, H, Z: even physical VGPR numbers of pairs (Z.hi must hold 0).  cm, c, bq, rare: SGPR pair
    operand names.  `rare` receives bq & ~c (lanes whose result needs the slow path)."""
    ch.add("v_mad_u64_u32 %s, vcc, %s, %s, 0" % (pair(T), a0, b0))
    ch.add("v_mov_b32 v%d, v%d" % (Z, T + 1))
    ch.add("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (pair(X), a0, b1, pair(Z)))
    ch.add("v_mad_u64_u32 %s, %s, %s, %s, %s" % (pair(X), cm, a1, b0, pair(X)), defs=[cm])
    ch.add("v_mov_b32 v%d, v%d" % (Z, X + 1))
    ch.add("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (pair(H), a1, b1, pair(Z)))
    ch.add("v_mov_b32 v%d, v%d" % (T + 1, X))
    ch.add("v_mad_u64_u32 %s, %s, v%d, -1, %s" % (pair(X), c, H, pair(T)), defs=[c])
    ch.add("v_subb_co_u32 v%d, %s, v%d, v%d, %s" % (X, bq, X, H + 1, cm), defs=[bq], uses=[cm])
    ch.add("v_cndmask_b32 v%d, 0, 1, %s" % (H, c), uses=[c])
    ch.add("v_subb_co_u32 v%d, %s, v%d, 0, %s" % (X + 1, bq, X + 1, bq), defs=[bq], uses=[bq])
    ch.add("v_mad_u64_u32 %s, vcc, v%d, -1, %s" % (pair(X), H, pair(X)))
    # SALU (own issue port): the borrow without a carry is the one case the sequence does not finish itself
    ch.add("s_andn2_b64 %s, %s, %s" % (rare, bq, c), defs=[], uses=[])


def addsub_chain(ch, u0, u1, t0, t1, S, D, k0, k1, out_s, out_d, sA, sB, sC, sD):
    """out_s <- weak(u + t), out_d <- weak(u - t); S, D: physical pairs for the raw sum / difference, k0 / k1: physical
    32-bit temporaries for the 0/1 carry and borrow; sC / sD receive the lanes that wrapped twice (slow path)."""
    ch.add("v_add_co_u32 v%d, %s, %s, %s" % (S, sA, u0, t0), defs=[sA])
    ch.add("v_sub_co_u32 v%d, %s, %s, %s" % (D, sB, u0, t0), defs=[sB])
    ch.add("v_addc_co_u32 v%d, %s, %s, %s, %s" % (S + 1, sA, u1, t1, sA), defs=[sA], uses=[sA])
    ch.add("v_subb_co_u32 v%d, %s, %s, %s, %s" % (D + 1, sB, u1, t1, sB), defs=[sB], uses=[sB])
    ch.add("v_cndmask_b32 v%d, 0, 1, %s" % (k0, sA), uses=[sA])
    ch.add("v_cndmask_b32 v%d, 0, 1, %s" % (k1, sB), uses=[sB])
    ch.add("v_mad_u64_u32 %s, %s, v%d, -1, %s" % (out_s, sC, k0, pair(S)), defs=[sC])       # + EPS where the sum wrapped
    ch.add("v_sub_co_u32 v%d, %s, v%d, v%d" % (D + 1, sD, D + 1, k1), defs=[sD])            # - EPS = - 2^32 + 1 where it borrowed
    ch.add("v_mad_u64_u32 %s, vcc, v%d, 1, %s" % (out_d, k1, pair(D)))


def interleave(chains):
    """Round-robin merge, then make sure every VALU read of an SGPR pair written by a VALU instruction has at least two
    instructions in between (s_nop otherwise)."""
    merged = []
    idx = [0] * len(chains)
    while any(i < len(c.ins) for i, c in zip(idx, chains)):
        for k, c in enumerate(chains):
            if idx[k] < len(c.ins):
                merged.append(c.ins[idx[k]])
                idx[k] += 1
    out = []
    last_def = {}
    for text, defs, uses in merged:
        need = 0
        for s in uses:
            if s in last_def:
                gap = len(out) - last_def[s] - 1
                need = max(need, 2 - gap)
        if need > 0:
            out.append(("s_nop %d" % (need - 1), (), ()))
            if need == 2:   # s_nop 1 = two wait states but one slot in our position count: count it twice
                out.append(("", (), ()))
        out.append((text, defs, uses))
        for s in defs:
            last_def[s] = len(out) - 1
    return [t for t, _, _ in out if t]


def asm_block(lines):
    return "\n".join('        "%s\\n\\t"' % l for l in lines[:-1]) + '\n        "%s"' % lines[-1]


def clobbers(lo, hi):
    return ", ".join('"v%d"' % r for r in range(lo, hi))


def gen_butterfly2():
    B = TEMP_BASE
    # chain A: T=B, X=B+2, H=B+4, Z=B+6 ; chain B: T=B+8, X=B+10, H=B+12, Z=B+14
    chains = []
    for k, base in enumerate((B, B + 8)):
        ch = Chain("bf%d" % k)
        T, X, H, Z = base, base + 2, base + 4, base + 6
        sfx = "ab"[k]
        mul_chain(ch, "%%[v%s0]" % sfx, "%%[v%s1]" % sfx, "%%[w%s0]" % sfx, "%%[w%s1]" % sfx, T, X, H, Z,
                  "%%[p%s]" % sfx, "%%[q%s]" % sfx, "%%[r%s]" % sfx, "%%[x%s]" % sfx)
        # the product sits in X; T and H are free again: raw sum in T, raw difference in H, 0/1 flags in Z.lo and X.lo/X.hi
        addsub_chain(ch, "%%[u%s0]" % sfx, "%%[u%s1]" % sfx, "v%d" % X, "v%d" % (X + 1), T, H, Z, X, "%%[s%s]" % sfx, "%%[d%s]" % sfx,
                     "%%[p%s]" % sfx, "%%[q%s]" % sfx, "%%[r%s]" % sfx, "%%[y%s]" % sfx)
        chains.append(ch)
    # NB addsub_chain uses k1 = X (v X.lo) as the borrow flag while t0 = X.lo is read by its first two instructions only
    lines = ["v_mov_b32 v%d, 0" % (B + 7), "v_mov_b32 v%d, 0" % (B + 15)] + interleave(chains)
    # the flag in Z.lo (k0) must not disturb Z.hi = 0; restore nothing: Z is re-zeroed at the top of every block
    lines += ["s_or_b64 %[xa], %[xa], %[ra]", "s_or_b64 %[xb], %[xb], %[rb]", "s_or_b64 %[xa], %[xa], %[ya]", "s_or_b64 %[xb], %[xb], %[yb]",
              "s_or_b64 %[xa], %[xa], %[xb]"]
    return lines, clobbers(B, B + 16)


def gen_addsub2():
    B = TEMP_BASE
    chains = []
    for k, base in enumerate((B, B + 6)):
        ch = Chain("as%d" % k)
        sfx = "ab"[k]
        addsub_chain(ch, "%%[u%s0]" % sfx, "%%[u%s1]" % sfx, "%%[v%s0]" % sfx, "%%[v%s1]" % sfx, base, base + 2, base + 4, base + 5,
                     "%%[s%s]" % sfx, "%%[d%s]" % sfx, "%%[p%s]" % sfx, "%%[q%s]" % sfx, "%%[r%s]" % sfx, "%%[y%s]" % sfx)
        chains.append(ch)
    lines = interleave(chains)
    lines += ["s_or_b64 %[ra], %[ra], %[ya]", "s_or_b64 %[rb], %[rb], %[yb]", "s_or_b64 %[ra], %[ra], %[rb]"]
    return lines, clobbers(B, B + 12)


# ---- multiplication by a compile-time power of two, and the butterfly around it (the shift-only DFT-16 of ntt_r16.hip) ----
P = 2**64 - 2**32 + 1
ROOT_2_32 = 0x185629DCDA58878C        # radix_2_subgroup_generator (gl.h: omega)
OMEGA16 = pow(ROOT_2_32, 1 << 28, P)  # gl::omega(4)
OMEGA16_T = [t for t in range(16) if pow(2, 12 * t, P) == OMEGA16][0]   # omega_16 = 2^(12 t), t odd


def w16_shift(e, inverse):
    """omega_16^(+-e) = (-1)^neg * 2^S: (S, neg)"""
    x = (12 * ((16 - OMEGA16_T) if inverse else OMEGA16_T) * e) % 192
    return x % 96, x >= 96


def shift_pairs():
    """the (S_a, S_b) pairs a radix-16 step runs side by side: equal exponents in the first three rounds, the exponent pairs
    (bitrev3(g), bitrev3(g + 1)) of the last one, forward and inverse; (0, 0) is addsub2"""
    pairs = set()
    for inverse in (False, True):
        for e in range(8):
            pairs.add((w16_shift(e, inverse)[0],) * 2)
        for ea, eb in ((0, 4), (2, 6), (1, 5), (3, 7)):
            pairs.add((w16_shift(ea, inverse)[0], w16_shift(eb, inverse)[0]))
    pairs.discard((0, 0))
    return sorted(pairs)


def shift_chain(ch, S, v0, v1, base, ct, bq):
    """X = v[base+2 : base+3] <- v * 2^S folded to 64 bits with 2^64 = 2^32 - 1, 2^96 = -1 (gl.h: mul_pow2_weak has the argument).
    With k = S mod 32 the product has three 32-bit limbs a = v0 << k, b = (v >> (32 - k)) & (2^32 - 1), c = v1 >> (32 - k) < 2^k at
    weights 2^S', 2^(S'+32), 2^(S'+64), S' = S - k.  Returns True when `ct` holds a carry the caller still owes: value = X + ct * 2^64."""
    T, X, C, E = base, base + 2, base + 4, base + 5
    k = S % 32
    if S < 32:        # a + b 2^32 + c 2^64 = (b : a) + c EPS
        ch.add("v_lshlrev_b32 v%d, %d, %s" % (T, k, v0))
        ch.add("v_alignbit_b32 v%d, %s, %s, %d" % (T + 1, v1, v0, 32 - k))
        ch.add("v_lshrrev_b32 v%d, %d, %s" % (C, 32 - k, v1))
        ch.add("v_mad_u64_u32 %s, %s, v%d, -1, %s" % (pair(X), ct, C, pair(T)), defs=[ct])
        return True
    if S < 64:        # a 2^32 + b 2^64 + c 2^96 = (a : 0) + b EPS - c;  a borrow of the subtraction (X < c < 2^28) goes to the slow path
        ch.add("v_mov_b32 v%d, 0" % T)
        ch.add("v_lshlrev_b32 v%d, %d, %s" % (T + 1, k, v0))
        ch.add("v_alignbit_b32 v%d, %s, %s, %d" % (E, v1, v0, 32 - k))
        ch.add("v_lshrrev_b32 v%d, %d, %s" % (C, 32 - k, v1))
        ch.add("v_mad_u64_u32 %s, %s, v%d, -1, %s" % (pair(X), ct, E, pair(T)), defs=[ct])
        ch.add("v_sub_co_u32 v%d, %s, v%d, v%d" % (X, bq, X, C), defs=[bq])
        ch.add("v_subb_co_u32 v%d, %s, v%d, 0, %s" % (X + 1, bq, X + 1, bq), defs=[bq], uses=[bq])
        return True
    # a 2^64 + b 2^96 + c 2^128 = a EPS - (c : b): no wrap in a EPS; where the difference borrows, D >= 2^64 - 2^52 and the
    # value is D - 2^64 = D - EPS = D - 2^32 + 1 (mod p), exact: the high word cannot borrow, the sum cannot wrap
    ch.add("v_lshlrev_b32 v%d, %d, %s" % (E, k, v0))
    ch.add("v_alignbit_b32 v%d, %s, %s, %d" % (T, v1, v0, 32 - k))
    ch.add("v_lshrrev_b32 v%d, %d, %s" % (T + 1, 32 - k, v1))
    ch.add("v_mad_u64_u32 %s, vcc, v%d, -1, 0" % (pair(X), E))
    ch.add("v_sub_co_u32 v%d, %s, v%d, v%d" % (X, bq, X, T), defs=[bq])
    ch.add("v_subb_co_u32 v%d, %s, v%d, v%d, %s" % (X + 1, bq, X + 1, T + 1, bq), defs=[bq], uses=[bq])
    ch.add("v_subb_co_u32 v%d, %s, v%d, 0, %s" % (X + 1, ct, X + 1, bq), defs=[ct], uses=[bq])     # - 2^32 where it borrowed (ct: no borrow out)
    ch.add("v_addc_co_u32 v%d, %s, v%d, 0, %s" % (X, bq, X, bq), defs=[bq], uses=[bq])             # + 1 where it borrowed
    ch.add("v_addc_co_u32 v%d, %s, v%d, 0, %s" % (X + 1, bq, X + 1, bq), defs=[bq], uses=[bq])
    return False


def addsub_carry_chain(ch, u0, u1, base, ct, out_s, out_d, sA, sB, sC, sD):
    """out_s <- weak(u + t), out_d <- weak(u - t) for t = X + ct * 2^64 (X = v[base+2 : base+3]): the owed carry joins the wrap of the
    sum and the borrow of the difference — (sA + ct) EPS is added, (sB + ct) EPS taken off — so it costs one instruction, not a
    correction of its own; a wrap of either correction goes to sC / sD (slow path), as in addsub_chain."""
    T, X, C, E, D = base, base + 2, base + 4, base + 5, base + 6
    ch.add("v_cndmask_b32 v%d, 0, 1, %s" % (E, ct), uses=[ct])
    ch.add("v_add_co_u32 v%d, %s, %s, v%d" % (T, sA, u0, X), defs=[sA])
    ch.add("v_sub_co_u32 v%d, %s, %s, v%d" % (D, sB, u0, X), defs=[sB])
    ch.add("v_addc_co_u32 v%d, %s, %s, v%d, %s" % (T + 1, sA, u1, X + 1, sA), defs=[sA], uses=[sA])
    ch.add("v_subb_co_u32 v%d, %s, %s, v%d, %s" % (D + 1, sB, u1, X + 1, sB), defs=[sB], uses=[sB])
    ch.add("v_addc_co_u32 v%d, vcc, v%d, 0, %s" % (C, E, sA), uses=[sA])
    ch.add("v_addc_co_u32 v%d, vcc, v%d, 0, %s" % (X, E, sB), uses=[sB])
    ch.add("v_mad_u64_u32 %s, %s, v%d, -1, %s" % (out_s, sC, C, pair(T)), defs=[sC])
    ch.add("v_sub_co_u32 v%d, %s, v%d, v%d" % (D + 1, sD, D + 1, X), defs=[sD])
    ch.add("v_mad_u64_u32 %s, vcc, v%d, 1, %s" % (out_d, X, pair(D)))


def gen_shiftbf2(SA, SB):
    B = TEMP_BASE
    chains = []
    rare = []
    for k, (S, base) in enumerate(((SA, B), (SB, B + 8))):
        ch = Chain("sb%d" % k)
        sfx = "ab"[k]
        o = lambda n: "%%[%s%s]" % (n, sfx)
        if S == 0:
            addsub_chain(ch, "%%[u%s0]" % sfx, "%%[u%s1]" % sfx, "%%[v%s0]" % sfx, "%%[v%s1]" % sfx, base, base + 2, base + 4, base + 5,
                         o("s"), o("d"), o("p"), o("q"), o("c"), o("e"))
        else:
            owed = shift_chain(ch, S, "%%[v%s0]" % sfx, "%%[v%s1]" % sfx, base, o("t"), o("r"))
            if owed:
                addsub_carry_chain(ch, "%%[u%s0]" % sfx, "%%[u%s1]" % sfx, base, o("t"), o("s"), o("d"), o("p"), o("q"), o("c"), o("e"))
            else:   # raw sum in T, raw difference in D, flags in C and X.lo (read by the first two instructions only)
                addsub_chain(ch, "%%[u%s0]" % sfx, "%%[u%s1]" % sfx, "v%d" % (base + 2), "v%d" % (base + 3), base, base + 6, base + 4, base + 2,
                             o("s"), o("d"), o("p"), o("q"), o("c"), o("e"))
            if 32 < S < 64:
                rare.append(o("r"))
        chains.append(ch)
    lines = interleave(chains)
    # SALU: the masks written last are read last (as in gen_butterfly2)
    for r in rare:
        lines.append("s_or_b64 %%[ca], %%[ca], %s" % r)
    lines += ["s_or_b64 %[ca], %[ca], %[cb]", "s_or_b64 %[ea], %[ea], %[eb]", "s_or_b64 %[ca], %[ca], %[ea]"]
    return lines, clobbers(B, B + 16)


HEADER = '''// GENERATED by tools/gen_gl_asm.py — do not edit.  Hand-scheduled gfx950 sequences for lazy Goldilocks arithmetic.
// Values are "weak" residues: any u64 congruent to the field element.  Every function returns a wave-uniform mask of the
// lanes (probability ~2^-32 per operation on random data) whose result the straight-line sequence did NOT finish: a
// second wrap of an addition / subtraction, or the borrow-without-carry case of the product (gl.h, mul_weak); the
// caller recomputes those through the canonical operators.  Temporaries are the fixed VGPRs v%d.. (clobbers).
#pragma once
'''


def main():
    b2, b2c = gen_butterfly2()
    a2, a2c = gen_addsub2()

    sh = ""
    for SA, SB in shift_pairs():
        lines, clob = gen_shiftbf2(SA, SB)
        sh += '''template <> __device__ __forceinline__ u64 shiftbf2_weak_asm<%d, %d>(u64 ua, u64 va, u64 ub, u64 vb, u64 &sa, u64 &da, u64 &sb, u64 &db) {
    u64 ta, ra, pa, qa, ca, ea, tb, rb, pb, qb, cb, eb;
    asm(
%s
        : [sa] "=&v"(sa), [da] "=&v"(da), [sb] "=&v"(sb), [db] "=&v"(db), [ta] "=&s"(ta), [ra] "=&s"(ra), [pa] "=&s"(pa), [qa] "=&s"(qa),
          [ca] "=&s"(ca), [ea] "=&s"(ea), [tb] "=&s"(tb), [rb] "=&s"(rb), [pb] "=&s"(pb), [qb] "=&s"(qb), [cb] "=&s"(cb), [eb] "=&s"(eb)
        : [ua0] "v"(lo32(ua)), [ua1] "v"(hi32(ua)), [va0] "v"(lo32(va)), [va1] "v"(hi32(va)),
          [ub0] "v"(lo32(ub)), [ub1] "v"(hi32(ub)), [vb0] "v"(lo32(vb)), [vb1] "v"(hi32(vb))
        : "vcc", "scc", %s);
    return ca;
}
''' % (SA, SB, asm_block(lines), clob)
    src = HEADER % TEMP_BASE
    src += '''
namespace gl {
#if defined(__HIP_DEVICE_COMPILE__)
// two radix-2 butterflies side by side:  (u, v) <- (u + v * w, u - v * w)  on weak residues
__device__ __forceinline__ u64 butterfly2_weak_asm(u64 ua, u64 va, u64 wa, u64 ub, u64 vb, u64 wb, u64 &sa, u64 &da, u64 &sb, u64 &db) {
    u64 pa, qa, ra, xa, ya, pb, qb, rb, xb, yb;
    asm(
%s
        : [sa] "=&v"(sa), [da] "=&v"(da), [sb] "=&v"(sb), [db] "=&v"(db), [pa] "=&s"(pa), [qa] "=&s"(qa), [ra] "=&s"(ra),
          [xa] "=&s"(xa), [ya] "=&s"(ya), [pb] "=&s"(pb), [qb] "=&s"(qb), [rb] "=&s"(rb), [xb] "=&s"(xb), [yb] "=&s"(yb)
        : [ua0] "v"(lo32(ua)), [ua1] "v"(hi32(ua)), [va0] "v"(lo32(va)), [va1] "v"(hi32(va)), [wa0] "v"(lo32(wa)), [wa1] "v"(hi32(wa)),
          [ub0] "v"(lo32(ub)), [ub1] "v"(hi32(ub)), [vb0] "v"(lo32(vb)), [vb1] "v"(hi32(vb)), [wb0] "v"(lo32(wb)), [wb1] "v"(hi32(wb))
        : "vcc", "scc", %s);
    return xa;
}
// the same without the multiplication (twiddle 1):  (u, v) <- (u + v, u - v)
__device__ __forceinline__ u64 addsub2_weak_asm(u64 ua, u64 va, u64 ub, u64 vb, u64 &sa, u64 &da, u64 &sb, u64 &db) {
    u64 pa, qa, ra, ya, pb, qb, rb, yb;
    asm(
%s
        : [sa] "=&v"(sa), [da] "=&v"(da), [sb] "=&v"(sb), [db] "=&v"(db), [pa] "=&s"(pa), [qa] "=&s"(qa), [ra] "=&s"(ra),
          [ya] "=&s"(ya), [pb] "=&s"(pb), [qb] "=&s"(qb), [rb] "=&s"(rb), [yb] "=&s"(yb)
        : [ua0] "v"(lo32(ua)), [ua1] "v"(hi32(ua)), [va0] "v"(lo32(va)), [va1] "v"(hi32(va)),
          [ub0] "v"(lo32(ub)), [ub1] "v"(hi32(ub)), [vb0] "v"(lo32(vb)), [vb1] "v"(hi32(vb))
        : "vcc", "scc", %s);
    return ra;
}
// two butterflies by compile-time powers of two side by side:  (u, v) <- (u + v * 2^S, u - v * 2^S)  on weak residues, for the pairs
// (SA, SB) the shift-only DFT-16 of ntt_r16.hip runs (S = 0: no product)
template <int SA, int SB> __device__ __forceinline__ u64 shiftbf2_weak_asm(u64 ua, u64 va, u64 ub, u64 vb, u64 &sa, u64 &da, u64 &sb, u64 &db);
%s#endif
// gl::omega(4) = 2^(12 t): the 16th root of unity of the twiddle tables as a power of two (checked in gl.h)
static constexpr int OMEGA16_LOG2_DIV12 = %d;
}  // namespace gl
''' % (asm_block(b2), b2c, asm_block(a2), a2c, sh, OMEGA16_T)
    old = open(OUT).read() if os.path.exists(OUT) else None
    if old != src:
        with open(OUT, "w") as f:
            f.write(src)
    return OUT


if __name__ == "__main__":
    print(main())
