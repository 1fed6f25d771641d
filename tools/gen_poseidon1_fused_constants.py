#!/usr/bin/env python3
"""Derive the fused partial-round constants of Poseidon (v1) over Goldilocks and emit them as a C data table
(era_boojum_amd/csrc/poseidon1_fused.inc), which the gate trace (gate_program.py) and the hand-written gate evaluator
(csrc/gate_poseidon.hip) both read.

The reference computes these tables at compile time (src/implementations/poseidon_goldilocks.rs:620-1010) by rewriting the
plain round sequence — AddRoundConstants / FullSBox / MulByMDS x 4, AddRoundConstants / PartialSBox / MulByMDSInPartialRound
x 21, the last partial round with MDS = M'' M', then 4 full rounds — in two passes:
  1. propagate_round_constants: move every round constant of the partial rounds (and of the first full round after them)
     backwards through the linear layers, merging the word-0 part into the preceding S-box ("S-box + constant for el 0");
  2. compute_equivalent_matrixes: push the M' factor backwards through every partial-round MDS, decomposing M' MDS again
     into M' M'' at each step (compute_poseidon_matrix_decomposition, :78-170);
and reads off (produce_optimied_params, :885-992): the constants added after the last full S-box, the dense matrix M' MDS
that follows them, one constant per partial S-box, and the first row (`v`) / first column (`w_hat`) of each M''.
This is that procedure, step for step, on the 360-entry round-constant table the kernels are built with and the circulant
MDS 2^MDS_MATRIX_EXPS.  Running the script twice gives the same file; the tests check the result against the permutation.

    python tools/gen_poseidon1_fused_constants.py
"""
import os
import re

P = (1 << 64) - (1 << 32) + 1
N = 12
HALF_FULL, PARTIAL = 4, 22
MDS_MATRIX_EXPS = [0, 0, 1, 0, 3, 5, 1, 8, 12, 3, 16, 10]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "era_boojum_amd", "csrc", "poseidon1_fused.inc")


def round_constants():
    txt = open(os.path.join(ROOT, "era_boojum_amd", "csrc", "poseidon_rc.inc")).read()
    vals = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)ULL", txt)]
    assert len(vals) == 360
    return [vals[N * r: N * r + N] for r in range(30)]


def mds():
    return [[1 << MDS_MATRIX_EXPS[(N - r + c) % N] for c in range(N)] for r in range(N)]


def identity():
    return [[1 if r == c else 0 for c in range(N)] for r in range(N)]


def transpose(a):
    return [[a[r][c] for r in range(N)] for c in range(N)]


def mat_vec(a, v):
    return [sum(a[r][c] * v[c] for c in range(N)) % P for r in range(N)]


def mat_mat(a, b):
    return [[sum(a[r][k] * b[k][c] for k in range(N)) % P for c in range(N)] for r in range(N)]


def inverse(a):
    lhs, rhs = [row[:] for row in a], identity()
    for d in range(N):
        inv = pow(lhs[d][d], P - 2, P)
        lhs[d] = [x * inv % P for x in lhs[d]]
        rhs[d] = [x * inv % P for x in rhs[d]]
        for r in range(N):
            if r != d:
                k = lhs[r][d]
                lhs[r] = [(x - k * y) % P for x, y in zip(lhs[r], lhs[d])]
                rhs[r] = [(x - k * y) % P for x, y in zip(rhs[r], rhs[d])]
    return rhs


def m_prime_form(a):                                   # poseidon_goldilocks.rs:108-128
    r = [row[:] for row in a]
    r[0][0] = 1
    for k in range(1, N):
        r[0][k] = 0
        r[k][0] = 0
    return r


def m_double_prime_form(a):                            # :130-170
    w = [0] + [a[k][0] for k in range(1, N)]
    w_hat = mat_vec(inverse(m_prime_form(a)), w)
    r = identity()
    r[0][0] = a[0][0]
    for k in range(1, N):
        r[0][k] = a[0][k]
        r[k][0] = w_hat[k]
    return r


def decompose(m):                                      # compute_poseidon_matrix_decomposition, :78-106: m == M'' M'
    t = transpose(m)
    mp, mpp = transpose(m_prime_form(t)), transpose(m_double_prime_form(t))
    assert mat_mat(mpp, mp) == [[x % P for x in row] for row in m]
    return mp, mpp


MDS = mds()
MDS_INV = inverse(MDS)
M_PRIME, M_DOUBLE_PRIME = decompose(MDS)


def default_structure(rc):                             # DEFAULT_ROUNDS_STRUCTURE, :623-678
    s = []
    for r in range(HALF_FULL):
        s += [("arc", tuple(rc[r])), ("full_sbox",), ("mds",)]
    for r in range(PARTIAL - 1):
        s += [("arc", tuple(rc[HALF_FULL + r])), ("partial_sbox",), ("mds_partial",)]
    s += [("arc", tuple(rc[HALF_FULL + PARTIAL - 1])), ("partial_sbox",), ("m_prime",), ("m_double_prime",)]
    for r in range(HALF_FULL):
        s += [("arc", tuple(rc[HALF_FULL + PARTIAL + r])), ("full_sbox",), ("mds",)]
    return s


def propagate_round_constants(structure):             # apply_optimization_deterministic_propagate_round_constants, :680-780
    s = list(structure)
    for idx in range(len(s) - 1, 1, -1):               # once: a constant behind M' M'' goes in front of them
        c, b, a = s[idx], s[idx - 1], s[idx - 2]
        if c[0] == "arc" and b[0] == "m_double_prime" and a[0] == "m_prime":
            s[idx], s[idx - 1], s[idx - 2] = b, a, ("arc", tuple(mat_vec(MDS_INV, c[1])))
    while True:
        new = list(s)
        for idx in range(len(new) - 1, 0, -1):
            b, a = new[idx], new[idx - 1]
            if a[0] == "partial_sbox" and b[0] == "arc":
                new[idx] = ("sbox_rc0", b[1][0])
                new[idx - 1] = ("arc", (0,) + b[1][1:])
            elif a[0] == "sbox_rc0" and b[0] == "arc":
                new[idx] = ("sbox_rc0", (a[1] + b[1][0]) % P)
                new[idx - 1] = ("arc", (0,) + b[1][1:])
            elif a[0] == "arc" and b[0] == "arc":
                new[idx] = ("arc", tuple((x + y) % P for x, y in zip(a[1], b[1])))
                new[idx - 1] = ("nop",)
            elif a[0] == "mds_partial" and b[0] == "arc":
                new[idx] = ("mds_partial",)
                new[idx - 1] = ("arc", tuple(mat_vec(MDS_INV, b[1])))
            elif b[0] == "nop":
                new[idx] = a
                new[idx - 1] = ("nop",)
        if new == s:
            return s
        s = new


def compute_equivalent_matrixes(structure):           # apply_optimization_deterministic_compute_equivalent_matrixes, :782-842
    s = list(structure)
    for idx in range(len(s) - 1, 0, -1):
        b, a = s[idx], s[idx - 1]
        if a[0] == "sbox_rc0" and b[0] in ("m_prime", "m_prime_explicit"):
            a, b = b, a
        elif a[0] == "mds_partial" and b[0] in ("m_prime", "m_prime_explicit"):
            mp = M_PRIME if b[0] == "m_prime" else b[1]
            new_mp, new_mpp = decompose(mat_mat(mp, MDS))
            a, b = ("m_prime_explicit", new_mp), ("m_double_prime_explicit", new_mpp)
        s[idx], s[idx - 1] = b, a
    return s


def optimized_structure(rc):
    s = propagate_round_constants(default_structure(rc))
    while s[0][0] == "nop":                            # CLEANED_DEFINITION, :848-874
        s = s[1:]
    return compute_equivalent_matrixes(s)


def produce_optimized_params(s):                      # produce_optimied_params, :885-992
    idx = HALF_FULL * 3 - 1
    assert s[idx][0] == "mds"
    idx += 1
    assert s[idx][0] == "arc"
    first = list(s[idx][1])
    fused_rc = mat_vec(MDS_INV, first)
    assert mat_vec(MDS, fused_rc) == first
    idx += 1
    assert s[idx][0] == "m_prime_explicit"
    dense = mat_mat(s[idx][1], MDS)
    idx += 1
    sbox_rc, vs, w_hats = [], [], []
    for _ in range(PARTIAL):
        assert s[idx][0] == "sbox_rc0"
        sbox_rc.append(s[idx][1])
        idx += 1
        mpp = s[idx][1] if s[idx][0] == "m_double_prime_explicit" else M_DOUBLE_PRIME
        assert s[idx][0] in ("m_double_prime_explicit", "m_double_prime") and all(mpp[j][j] == 1 for j in range(N))
        vs.append([mpp[0][k + 1] for k in range(N - 1)])
        w_hats.append([mpp[k + 1][0] for k in range(N - 1)])
        idx += 1
    assert s[idx][0] == "full_sbox"
    return fused_rc, dense, sbox_rc, vs, w_hats


def fused_constants():
    return produce_optimized_params(optimized_structure(round_constants()))


def apply(structure, state):
    """Runs an operation sequence over a state (Operation::apply_over_state, :566-608): for the self-check below."""
    st = [x % P for x in state]
    for op in structure:
        k = op[0]
        if k == "arc":
            st = [(x + c) % P for x, c in zip(st, op[1])]
        elif k == "full_sbox":
            st = [pow(x, 7, P) for x in st]
        elif k == "partial_sbox":
            st[0] = pow(st[0], 7, P)
        elif k == "sbox_rc0":
            st[0] = (pow(st[0], 7, P) + op[1]) % P
        elif k in ("mds", "mds_partial"):
            st = mat_vec(MDS, st)
        elif k == "m_prime":
            st = mat_vec(M_PRIME, st)
        elif k == "m_double_prime":
            st = mat_vec(M_DOUBLE_PRIME, st)
        elif k in ("m_prime_explicit", "m_double_prime_explicit"):
            st = mat_vec(op[1], st)
    return st


def emit(path=OUT):
    fused_rc, dense, sbox_rc, vs, w_hats = fused_constants()
    rc = round_constants()
    s0, s1 = default_structure(rc), optimized_structure(rc)
    for seed in range(4):                              # test_valid_transformation, :1035-1050
        st = [(seed * 0x9E3779B97F4A7C15 + 7 * k + 1) % P for k in range(N)]
        assert apply(s0, st) == apply(s1, st)

    def table(name, vals):
        lines = ["#define %s { \\" % name]
        for i in range(0, len(vals), 4):
            lines.append("  " + ", ".join("0x%016xULL" % v for v in vals[i:i + 4]) + (", \\" if i + 4 < len(vals) else " \\"))
        return lines + ["}"]
    out = ["/* GENERATED by tools/gen_poseidon1_fused_constants.py — do not edit.  Poseidon (v1) over Goldilocks, fused partial",
           " * rounds: the tables the reference derives at compile time (src/implementations/poseidon_goldilocks.rs:620-1010).",
           " *   BJ_P1_FUSED_RC          ROUND_CONSTANTS_FUZED_LAST_FULL_AND_FIRST_PARTIAL [12]",
           " *   BJ_P1_FUSED_DENSE       FUZED_DENSE_MATRIX_LAST_FULL_AND_FIRST_PARTIAL [12][12], row-major",
           " *   BJ_P1_FUSED_SBOX_RC     ROUND_CONSTANTS_FOR_FUZED_SBOXES [22]",
           " *   BJ_P1_FUSED_VS          VS_FOR_PARTIAL_ROUNDS [22][11]",
           " *   BJ_P1_FUSED_W_HATS      W_HATS_FOR_PARTIAL_ROUNDS [22][11] */",
           "#ifndef BJ_POSEIDON1_FUSED_INC", "#define BJ_POSEIDON1_FUSED_INC"]
    out += table("BJ_P1_FUSED_RC", fused_rc)
    out += table("BJ_P1_FUSED_DENSE", [x for row in dense for x in row])
    out += table("BJ_P1_FUSED_SBOX_RC", sbox_rc)
    out += table("BJ_P1_FUSED_VS", [x for row in vs for x in row])
    out += table("BJ_P1_FUSED_W_HATS", [x for row in w_hats for x in row])
    out += ["#endif", ""]
    txt = "\n".join(out)
    if not os.path.exists(path) or open(path).read() != txt:
        with open(path, "w") as f:
            f.write(txt)
    return path


if __name__ == "__main__":
    print(emit())
