"""Inputs and the Python model for the butterflies by 16th roots of unity (csrc/gl.h: mul_pow2_weak, w16_butterfly_weak,
w16_butterfly2_weak; operator 32 of bj_field_op_batch).  omega_16 = gl::omega(4) is a power of two, so (u, v) <- (u + v w, u - v w) for
w = omega_16^(+-e) needs no product; the model below is Python integers mod p and knows nothing of the limbs.  BRANCH names, for a
word v and a shift S, which branch of gl.h's limb algorithm v takes — the tests use it to prove the vectors reach every branch."""
import random

P = 2**64 - 2**32 + 1
EPS = 2**32 - 1
M64 = 2**64 - 1
OMEGA16 = pow(0x185629DCDA58878C, 1 << 28, P)          # gl::omega(4)
SHIFTS = (12, 24, 36, 48, 60, 72, 84)
# operator 32's selector: 0..7 -> (e, e); 8..11 -> the pairs of a step's last round
PAIRS = [(e, e) for e in range(8)] + [(0, 4), (2, 6), (1, 5), (3, 7)]

EDGE = [0, 1, P - 1, P, P + 1, 2**32 - 1, 2**32, 2**64 - 2**32, 2**64 - 1]


def root(e, inverse):
    return pow(OMEGA16, (16 - e) % 16 if inverse else e, P)


def butterfly(u, v, e, inverse):
    t = v * root(e, inverse) % P
    return (u + t) % P, (u - t) % P


def branch(v, S):
    """the branch of gl::mul_pow2_weak<S>(v): 'plain', 'wrap' (S < 32), 'carry' / 'borrow' (32 < S < 64), 'borrow' (S > 64)"""
    k = S % 32
    a, b, c = (v << k) & 0xFFFFFFFF, (v >> (32 - k)) & 0xFFFFFFFF, v >> (64 - k)
    if S < 32:
        return "wrap" if (b << 32 | a) + c * EPS > M64 else "plain"
    if S < 64:
        full = (a << 32) + b * EPS
        cy, r = full > M64, full & M64
        bw = r < c
        return "plain" if cy == bw else "carry" if cy else "borrow"
    return "borrow" if a * EPS < (c << 32 | b) else "plain"


BRANCHES = {S: ("plain", "wrap") if S < 32 else ("plain", "carry", "borrow") if S < 64 else ("plain", "borrow") for S in SHIFTS}


def branch_words():
    """for every shift, words v that take each branch of the product, found by construction (borrows) and by a seeded search"""
    rng = random.Random(0x16)
    out = []
    for S in SHIFTS:
        k = S % 32
        want = set(BRANCHES[S])
        found = {}
        cand = [((1 << k) - 1) << (64 - k), 1 << 63, 1 << (64 - k), (1 << 32) | 1, 1 << 32, M64, P - 1]
        cand += [rng.getrandbits(64) for _ in range(4000)]
        cand += [(rng.getrandbits(k) << (64 - k)) | rng.getrandbits(2) for _ in range(64)]        # high limb alone: the borrows
        for v in cand:
            br = branch(v, S)
            if len(found.setdefault(br, [])) < 4:
                found[br].append(v)
        assert set(found) == want, (S, sorted(found))
        for ws in found.values():
            out += ws
    return out


def pairs(n_random=3000):
    """(u, v) pairs: the edge grid, every branch word against the u that make the sum wrap, the difference borrow, both or neither
    (and the second wraps the device sequences hand to their slow path), and seeded random pairs"""
    rng = random.Random(0x5EED16)
    ps = [(u, v) for u in EDGE for v in EDGE]
    us = EDGE + [2**63, 2**64 - 2**31, 2**33, 0xFFFFFFFE00000003, rng.getrandbits(64), rng.getrandbits(64)]
    for v in branch_words():
        ps += [(u, v) for u in us]
    ps += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(n_random)]
    return ps
