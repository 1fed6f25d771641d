"""Inputs shared by the stage-operator tests: the satisfied circuit and oracle LDEs of tests/test_gpu_stage_ops.py (also what
tests/test_quotient_ref.py pins the python restatement on), and the arbitrary columns, challenges and case lists of
tests/test_gpu_quotient_terms.py — here, so that the CPU test can check properties of the very inputs the GPU test runs
(no zero denominator in the bj_lookup_polys cases).  Nothing in this module touches the GPU."""
import numpy as np

import oracle as O
from era_boojum_amd import synthetic as S
from oracle import prover as OP

P = O.P

BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (77, P - 5)
LBETA, LGAMMA = (P - 1, 3), (0xDEADBEEFCAFEF00D % P, 0x1111111122222222)
ALPHA = (0x9E3779B97F4A7C15 % P, 0xBF58476D1CE4E5B9 % P)


# ------------------------------------------------------------------------------ a satisfied circuit and its LDEs by the oracle
def circuit(log_n, **kw):
    c = S.sha_shaped_circuit(log_n, seed=31 + log_n, table_bits=2, **kw)
    S.check_satisfied(c)
    return c


def lookup_vars(c):
    """The lookup sub-arguments' variable columns: width per sub-argument, width + 1 with the table id as a variable."""
    return np.ascontiguousarray(c.variables[c.num_gp_vars:c.num_gp_vars + c.lookup_reps * c.lookup_cols_per_sub])


def quotient_inputs(c):
    """LDEs of every column the quotient reads, restricted to the first q cosets, by the oracle; plus the alpha powers."""
    log_n, q, V = c.log_n, c.quotient_degree, c.num_vars
    log_q = q.bit_length() - 1
    Q = c.n * q
    z, partials = OP.copy_perm_stage2(c.variables, c.sigmas, c.non_residues, log_n, q, BETA, GAMMA, threads=8)
    stage2 = [z[0], z[1]] + [partials[j][k] for j in range(partials.shape[0]) for k in range(2)]
    reps, w = c.lookup_reps, c.lookup_width
    A, B = OP.lookup_polys(lookup_vars(c), OP.lookup_table_id(c, c.constants), c.tables, c.multiplicities[0], reps, w, log_n, LBETA, LGAMMA,
                           threads=8)
    stage2 += [A[i][k] for i in range(reps) for k in range(2)] + [B[0], B[1]]

    def lde_q(cols):
        cols = np.ascontiguousarray(np.stack(cols) if isinstance(cols, list) else cols)
        return np.ascontiguousarray(O.lde_batch(O.ifft_batch(cols, 1, threads=8), log_q, threads=8).reshape(cols.shape[0], Q))
    d = dict(vars=lde_q(c.variables), mult=lde_q(c.multiplicities[:1])[0], sig=lde_q(c.sigmas), con=lde_q(c.constants),
             tab=lde_q(c.tables), s2=lde_q(stage2))
    n_part = partials.shape[0]
    d["n_part"], d["Q"], d["log_q"] = n_part, Q, log_q
    n_lookup, n_gate = reps + 1, sum(g.reps * g.num_terms for g in c.gates)
    n_chunks = (V + q - 1) // q
    al = [(1, 0)]
    while len(al) < n_lookup + n_gate + 1 + n_chunks:
        al.append(OP.emul(al[-1], ALPHA))
    d["alphas"], d["n_lookup"], d["n_gate"], d["n_chunks"] = al, n_lookup, n_gate, n_chunks
    return d


def oracle_quotient(c, d, alphas):
    s2, n_part, reps = d["s2"], d["n_part"], c.lookup_reps
    o = 2 + 2 * n_part
    return OP.quotient(d["vars"], d["con"], d["sig"], np.ascontiguousarray(s2[0:2]), np.ascontiguousarray(s2[2:o]),
                       np.ascontiguousarray(s2[o:o + 2 * reps]), np.ascontiguousarray(s2[o + 2 * reps:]), d["mult"], d["tab"], c,
                       d["log_q"], alphas, BETA, GAMMA, LBETA, LGAMMA, threads=8)


# ------------------------------------------------------------------------------ arbitrary words
# the words around every boundary of the arithmetic: 0, 1, p - 1, p, p + 1, 2^32 - 1, 2^32, 2^64 - 2^32, 2^64 - 1
EDGE_WORDS = [0, 1, P - 1, P, P + 1, 2**32 - 1, 2**32, 2**64 - 2**32, 2**64 - 1]
NONCANONICAL_SHARE = 0.25


def raw_columns(rng, cols, stride, points, salt=0):
    """[cols][stride] random uint64 words, no circuit behind them.  A quarter of them is in [p, 2^64).  Over the first `points`
    words of every column the nine EDGE_WORDS are planted at known lanes: word k on the lone lane 5 + 7 k of every column (a
    whole row of that word), and across the whole wave of 64 lanes 64 (k + 1) .. 64 (k + 2) — there column c holds word k + c +
    salt (mod 9), so a wave sees a different edge word in every column and, given 640 points, every column every word.  A
    one-point column holds an edge word.  The words behind `points` are random as well."""
    a = rng.integers(0, P, size=(cols, stride), dtype=np.uint64)
    over = rng.random(size=a.shape) < NONCANONICAL_SHARE
    a = np.where(over, np.uint64(P) + rng.integers(0, 2**32 - 1, size=a.shape, dtype=np.uint64), a)
    for k in range(9):
        if 5 + 7 * k < points:
            a[:, 5 + 7 * k] = np.uint64(EDGE_WORDS[(k + salt) % 9])
        lo, hi = 64 * (k + 1), min(64 * (k + 2), points)
        for c in range(cols if lo < hi else 0):
            a[c, lo:hi] = np.uint64(EDGE_WORDS[(k + c + salt) % 9])
    if points == 1:
        for c in range(cols):
            a[c, 0] = np.uint64(EDGE_WORDS[(c + salt) % 9])
    return a


def raw_scalar(rng, noncanonical):
    """one challenge word: a residue, or a word in [p, 2^64)"""
    return P + int(rng.integers(0, 2**32 - 1)) if noncanonical else int(rng.integers(0, P, dtype=np.uint64))


def raw_challenge(rng, noncanonical):
    return (raw_scalar(rng, noncanonical), raw_scalar(rng, noncanonical))


def raw_alphas(rng, count, noncanonical):
    """`count` F_p^2 challenge words; non-canonical: every word in [p, 2^64), 2^64 - 1 and p among them"""
    al = [raw_challenge(rng, noncanonical) for _ in range(count)]
    if noncanonical and count:
        al[0] = (2**64 - 1, P)
        al[-1] = (al[-1][0], 2**64 - 1)
    return al


# ------------------------------------------------------------------------------ the bj_lookup_polys cases
LOOKUP_WIDTHS, LOOKUP_REPS = (1, 2, 4, 7, 8), (1, 3, 11)
LOOKUP_POLYS_LOG_N, LOOKUP_POLYS_GAP = 8, 24


def lookup_polys_case(w, reps, tid_var, noncanonical):
    """Columns at a stride above n = 2^8 and challenges for one bj_lookup_polys case (tests/test_quotient_ref.py asserts that no
    denominator of any case is zero): dict(lvars, tid, tables, mult, lbeta, lgamma, stride, n)."""
    n = 1 << LOOKUP_POLYS_LOG_N
    stride = n + LOOKUP_POLYS_GAP
    rng = np.random.default_rng([w, reps, int(tid_var), int(noncanonical), 77])
    cps = w + 1 if tid_var else w
    return dict(lvars=raw_columns(rng, reps * cps, stride, n, salt=w), tid=None if tid_var else raw_columns(rng, 1, stride, n, salt=3)[0],
                tables=raw_columns(rng, w + 1, stride, n, salt=reps), mult=raw_columns(rng, 1, stride, n, salt=5)[0],
                lbeta=raw_challenge(rng, noncanonical), lgamma=raw_challenge(rng, noncanonical), stride=stride, n=n)


def lookup_polys_cases():
    return [(w, reps, tid_var, nc) for w in LOOKUP_WIDTHS for reps in LOOKUP_REPS for tid_var in (False, True) for nc in (False, True)]
