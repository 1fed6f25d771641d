"""Inputs that drive the S-box products of the Poseidon kernels into the rare branches of gl::mul_weak (csrc/gl.h): the fixture
of tools/find_poseidon_sbox_rare.c (tests/golden/poseidon_sbox_rare.json) and the constructions that place one of its values at
a chosen S-box input, in python integers.

  * v1 permutation (csrc/poseidon1.hip): `v1_construct` inverts the rounds from the target round back to round 0 on residues
    (inverse circulant MDS, S-box inverse x^(7^-1 mod p-1), minus the constants); `v1_forward` restates the permutation and
    logs every S-box input.
  * v1 tree leaves and nodes (capacity words 0): round 0 through the rate words (`tree_round0_word`), round 1 by solving one
    row of the MDS for one rate word (`tree_round1_words`).
  * flattened gates (csrc/gate_poseidon.hip): every reset variable feeds an S-box, through + RC or
    directly; round 0 comes from the 12 inputs (+ RC for v1, Poseidon2's external matrix first, then + RC).
"""
import json
import os

import numpy as np

import oracle as O

P = O.P
M64 = (1 << 64) - 1
EPS = 0xFFFFFFFF
PRODUCTS = ("x*x", "x2*x", "x2*x2", "x4*x3")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_sbox_rare.json")

RC = [[int(x) for x in row] for row in O.poseidon_round_constants()]     # (30, 12), the table both permutations use
EXPS = [0, 0, 1, 0, 3, 5, 1, 8, 12, 3, 16, 10]
MDS = [[1 << EXPS[(c - r) % 12] for c in range(12)] for r in range(12)]
E7 = pow(7, -1, P - 1)                                                  # x -> x^7 is a bijection: gcd(7, p - 1) = 1


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["entries"]


def entries(chain, cls):
    return [e for e in fixture() if e["chain"] == chain and e["class"] == cls]


# ---- mul_weak on 64-bit words: the model of tools/find_poseidon_sbox_rare.c
def mul_weak_model(a, b):
    """(weak result, class): class bit0 = the final subtraction borrows, bit1 = the reduction multiply-add carries."""
    a0, a1, b0, b1 = a & EPS, a >> 32, b & EPS, b >> 32
    T = a0 * b0
    X = a1 * b0 + a0 * b1 + (T >> 32)
    cm, X = X >> 64, X & M64
    H = a1 * b1 + (X >> 32)
    R = (H & EPS) * EPS + ((T & EPS) | ((X & EPS) << 32))
    c, R = R >> 64, R & M64
    D = R - (H >> 32) - cm
    bo, D = int(D < 0), D & M64
    if bo and not c:
        D = (D - EPS) & M64
    return (D + c * EPS) & M64, bo | (c << 1)


def pow7_operands(x, chain, mul=None):
    """The operand pairs of the four products of x^7 as the device forms them: 'weak' (p1_pow7, results passed on unreduced)
    or 'canonical' (the gates' pow7, canon after every product).  `mul(a, b) -> weak result` defaults to the model."""
    mul = mul or (lambda a, b: mul_weak_model(a, b)[0])
    fix = (lambda v: v % P) if chain == "canonical" else (lambda v: v)
    x2 = fix(mul(x, x))
    x3, x4 = fix(mul(x2, x)), fix(mul(x2, x2))
    return [(x, x), (x2, x), (x2, x2), (x4, x3)]


# ---- the v1 permutation on residues
def _matvec(M, s):
    return [sum(m * v for m, v in zip(row, s)) % P for row in M]


def solve_mod_p(M, rhs):
    n = len(M)
    A = [list(row) + [rhs[i] % P] for i, row in enumerate(M)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] % P)
        A[c], A[piv] = A[piv], A[c]
        inv = pow(A[c][c], P - 2, P)
        A[c] = [x * inv % P for x in A[c]]
        for r in range(n):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [(x - f * y) % P for x, y in zip(A[r], A[c])]
    return [A[i][n] for i in range(n)]


def _inverse(M):
    n = len(M)
    cols = [solve_mod_p(M, [int(i == j) for i in range(n)]) for j in range(n)]
    return [[cols[j][i] for j in range(n)] for i in range(n)]


MDS_INV = _inverse(MDS)


def is_full(r):
    return r < 4 or r >= 26


def v1_forward(state):
    """poseidon_goldilocks_naive.rs round by round: (output, S-box inputs per round; partial rounds use word 0 only)."""
    s, log = [x % P for x in state], []
    for r in range(30):
        s = [(x + RC[r][k]) % P for k, x in enumerate(s)]
        log.append(list(s))
        s = [pow(x, 7, P) if (is_full(r) or k == 0) else x for k, x in enumerate(s)]
        s = _matvec(MDS, s)
    return s, log


def v1_construct(round_, words, x, rng):
    """A state whose S-box input at round `round_` is x in every word of `words` (word 0 only in a partial round), the other
    words of that round random: the rounds inverted back to round 0."""
    u = [int(rng.integers(0, P, dtype=np.uint64)) for _ in range(12)]
    for k in words:
        u[k] = x
    for r in range(round_, -1, -1):                       # u = S-box input of round r
        s = [(v - RC[r][k]) % P for k, v in enumerate(u)]
        if r == 0:
            return s
        y = _matvec(MDS_INV, s)                           # S-box output of round r - 1
        u = [pow(v, E7, P) if (is_full(r - 1) or k == 0) else v for k, v in enumerate(y)]


def tree_round0_word(k, x):
    """The rate word k that makes round 0 see x at word k (capacity words 0)."""
    return (x - RC[0][k]) % P


def tree_round1_words(j, x, rng, free=8):
    """`free` rate words (the rest 0: capacity and zero padding) whose permutation sees x at the round-1 S-box of word j: the
    round-0 S-box outputs z_k of the rate words are random but one, which solves row j of the MDS (its coefficient is a power
    of two), and the rate words are their seventh roots minus the constants."""
    z = [pow(RC[0][k], 7, P) for k in range(12)]          # word k = 0: (0 + rc)^7
    m = (j + 3) % free                                    # the solved word
    for k in range(free):
        if k != m:
            z[k] = int(rng.integers(0, P, dtype=np.uint64))
    rest = sum(MDS[j][k] * z[k] for k in range(12) if k != m)
    z[m] = ((x - RC[1][j]) - rest) * pow(MDS[j][m], P - 2, P) % P
    return [(pow(z[k], E7, P) - RC[0][k]) % P for k in range(free)]


# ---- the flattened gates: 12 inputs, 12 outputs, then one variable per reset S-box input
# slots: ("full", r) for r in 0-3 and 26-29, ("partial", p) for p in 0-21
SLOTS = [("full", r) for r in range(4)] + [("partial", p) for p in (0, 10, 21)] + [("full", r) for r in range(26, 30)]
M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]
EXT = [[M4[i % 4][j % 4] * (2 if i // 4 == j // 4 else 1) for j in range(12)] for i in range(12)]


def _full_var(r, i):
    return i if r == 0 else (24 + 12 * (r - 1) + i if r < 4 else 82 + 12 * (r - 26) + i)


def gate_sbox_var(gate, slot, i):
    """(variable index, constant added before the S-box) of S-box input i of `slot`; None for round 0 (from the inputs)."""
    kind, r = slot
    if kind == "partial":
        return 60 + r, 0
    if r == 0:
        return None
    if gate == "v1" and r == 26:
        return _full_var(r, i), 0                       # v1 round 26: its constants went into the partial rounds
    return _full_var(r, i), RC[r][i]


def p2_ext_mds(s):
    """The external layer of Poseidon2 as the kernels compute it (three M4 blocks, then each column sum added): a second form
    of EXT, to check the round-0 solve."""
    out = []
    for b in range(3):
        x = s[4 * b:4 * b + 4]
        out += [sum(M4[i][k] * x[k] for k in range(4)) % P for i in range(4)]
    sums = [(out[j] + out[4 + j] + out[8 + j]) % P for j in range(4)]
    return [(out[i] + sums[i % 4]) % P for i in range(12)]


def gate_sbox_inputs(gate, v, slot):
    """The 12 S-box inputs of a full-round slot (1 of a partial slot) restated from the variables."""
    v = [x % P for x in v]
    kind, r = slot
    if kind == "full" and r == 0:
        s = v[:12] if gate == "v1" else p2_ext_mds(v[:12])
        return [(s[i] + RC[0][i]) % P for i in range(12)]
    n = 1 if kind == "partial" else 12
    return [(v[gate_sbox_var(gate, slot, i)[0]] + gate_sbox_var(gate, slot, i)[1]) % P for i in range(n)]


def gate_point(gate, targets, rng):
    """130 canonical variables, random but for `targets` = [(slot, word, x)]: the S-box input `word` of `slot` is x."""
    v = [int(x) for x in rng.integers(0, P, size=130, dtype=np.uint64)]
    r0 = {}
    for slot, i, x in targets:
        sv = gate_sbox_var(gate, slot, i)
        if sv is None:
            r0[i] = x
        else:
            v[sv[0]] = (x - sv[1]) % P
    if r0:
        want = [r0.get(i, (v[i] + RC[0][i]) % P) for i in range(12)]
        rhs = [(w - RC[0][i]) % P for i, w in enumerate(want)]
        v[:12] = rhs if gate == "v1" else solve_mod_p(EXT, rhs)
    return v
