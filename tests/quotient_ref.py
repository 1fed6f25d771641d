"""The quotient-term operators and the lookup polynomials restated from their definitions in python integers (numpy object
arrays: exact, a few thousand points at most).  Nothing here comes from oracle/prover_ops.c or from the library: the domain is
built from the generator 7, the gates from their formulas, F_p^2 = F_p[u] / (u^2 - 7) from its multiplication rule.
tests/test_quotient_ref.py pins every function against the oracle on a satisfied circuit; tests/test_gpu_quotient_terms.py
compares the device with it on arbitrary columns.

Inputs are raw uint64 words of any value (columns as [cols][>= points] arrays, challenges as (c0, c1) pairs of words) and are
reduced mod p first; outputs are canonical residues (uint64)."""
import numpy as np

P = 2**64 - 2**32 + 1
GEN = 7                                   # multiplicative generator = LDE coset shift = the non-residue of F_p^2
ROOT_2_32 = pow(GEN, (P - 1) >> 32, P)    # generates the subgroup of order 2^32

KIND_CONSTANT_ALLOCATOR, KIND_FMA, KIND_REDUCTION4, KIND_NOP = 1, 2, 3, 4
OP_ADD, OP_DOUBLE, OP_SUB, OP_NEGATE, OP_MUL, OP_SQUARE, OP_INVERSE = range(1, 8)   # bj_gate_program (include/boojum_hip.h)
IDX_VARIABLE, IDX_WITNESS, IDX_CONSTANT_POLY, IDX_TEMPORARY, IDX_VALUE = range(5)


# ---------------------------------------------------------------------------------------------- field helpers
def res(words):
    """raw uint64 words -> object array of residues"""
    return np.asarray(words, dtype=np.uint64).astype(object) % P


def e2(ch):
    return (int(ch[0]) % P, int(ch[1]) % P)


def to_words(*cols):
    return np.stack([np.asarray(c % P, dtype=object).astype(np.uint64) for c in cols])


def inv(x):
    """elementwise x^(p-2); 0 stays 0"""
    if isinstance(x, np.ndarray):
        return np.array([pow(int(v), P - 2, P) for v in x.reshape(-1)], dtype=object).reshape(x.shape)
    return pow(int(x), P - 2, P)


def emul(a, b): return ((a[0] * b[0] + GEN * (a[1] * b[1])) % P, (a[0] * b[1] + a[1] * b[0]) % P)
def eadd(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def esub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def escale(a, s): return (a[0] * s % P, a[1] * s % P)


def einv(a):
    ni = inv((a[0] * a[0] - GEN * (a[1] * a[1])) % P)     # 1 / (a0 + a1 u) = (a0 - a1 u) / (a0^2 - 7 a1^2)
    return (a[0] * ni % P, (-a[1]) * ni % P)


def epowers(g, count):
    out = [(1, 0)]
    while len(out) < count:
        out.append(emul(out[-1], g))
    return out


# ---------------------------------------------------------------------------------------------- domain
def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def omega(log_size):
    return pow(ROOT_2_32, 1 << (32 - log_size), P)


def lde_points(log_n, log_lde, first, count):
    """x_I = 7 * w_N^bitrev(I), N = n << log_lde, for the flat indices I = coset * n + i in first .. first + count"""
    log_N = log_n + log_lde
    w = omega(log_N)
    return np.array([GEN * pow(w, bitrev(I, log_N), P) % P for I in range(first, first + count)], dtype=object)


def coset_xn(log_n, log_lde, coset):
    """x^n on a coset: 7^n * w_L^bitrev_L(coset)"""
    return pow(GEN, 1 << log_n, P) * pow(omega(log_lde), bitrev(coset, log_lde), P) % P


def next_in_coset(I, log_n):
    """flat index of omega * x_I: the next natural index inside the same coset"""
    n = 1 << log_n
    return (I // n) * n + bitrev((bitrev(I % n, log_n) + 1) % n, log_n)


# ---------------------------------------------------------------------------------------------- gate terms
def selector(consts, path, Q):
    sel = np.ones(Q, dtype=object)
    for b, bit in enumerate(path):
        c = res(consts[b][:Q])
        sel = sel * (c if bit else (1 - c)) % P
    return sel


def _run_program(prog, var, con):
    """The op list of a bj_gate_program on columns: var(i), con(i) give the columns of one repetition."""
    tmp = {}

    def get(ix):
        k, i = ix
        if k == IDX_VARIABLE: return var(i)
        if k == IDX_CONSTANT_POLY: return con(i)
        if k == IDX_TEMPORARY: return tmp[i]
        assert k == IDX_VALUE
        return int(prog.values[i]) % P
    for op, dst, a, b in prog.relations:
        x = get(a)
        if op == OP_ADD: r = x + get(b)
        elif op == OP_DOUBLE: r = 2 * x
        elif op == OP_SUB: r = x - get(b)
        elif op == OP_NEGATE: r = -x
        elif op == OP_MUL: r = x * get(b)
        elif op == OP_SQUARE: r = x * x
        else: r = inv(x)
        tmp[dst] = r % P
    return [get(w) for w in prog.writes]


def gate_terms(vars, consts, g, Q):
    """term_{g,r,t} for every repetition r and term t of one gate, in the order the alpha powers are spent: a list of arrays"""
    pl, out = len(g.path), []
    for r in range(g.reps):
        def v(k, r=r): return res(vars[r * g.var_stride + k][:Q])
        if g.kind == KIND_CONSTANT_ALLOCATOR:
            out.append((v(0) - res(consts[pl + r * g.const_stride][:Q])) % P)
        elif g.kind == KIND_FMA:                               # k0 a b + k1 c - d, k0 and k1 shared by the row
            k0, k1 = res(consts[pl][:Q]), res(consts[pl + 1][:Q])
            out.append((k0 * v(0) * v(1) + k1 * v(2) - v(3)) % P)
        elif g.kind == KIND_REDUCTION4:                        # sum k_i v_i - v_4
            out.append((sum(res(consts[pl + i][:Q]) * v(i) for i in range(4)) - v(4)) % P)
        else:
            def c(k, r=r): return res(consts[pl + r * g.const_stride + k][:Q])
            out += [np.broadcast_to(np.asarray(t, dtype=object), (Q,)) % P for t in _run_program(g.program, v, c)]
    return out


def gates_term(vars, consts, gates, alphas, Q):
    """T[I] = sum_g sel_g(I) * sum_r alpha_{g,r} * term_{g,r}(I); one F_p^2 power per (gate, repetition, term) in gate order"""
    T = (np.zeros(Q, dtype=object), np.zeros(Q, dtype=object))
    a = 0
    for g in gates:
        if g.kind == KIND_NOP or g.num_terms == 0:
            continue
        if g.kind >= 5 and getattr(g, "program", None) is None:   # evaluated elsewhere: its powers are spent all the same
            a += g.reps * g.num_terms
            continue
        s = (np.zeros(Q, dtype=object), np.zeros(Q, dtype=object))
        for term in gate_terms(vars, consts, g, Q):
            s = eadd(s, escale(e2(alphas[a]), term))
            a += 1
        T = eadd(T, escale(s, selector(consts, g.path, Q)))
    assert a <= len(alphas)
    return T


# ---------------------------------------------------------------------------------------------- lookup
def lookup_denominators(lvars, table_id, tables, reps, w, lbeta, lgamma, Q):
    """lbeta + sum_j lgamma^j col_ij (+ lgamma^w tid) for the reps sub-arguments, then lbeta + sum_{j<=w} lgamma^j tab_j.
    table_id None: the id is the last of the w + 1 variable columns of every sub-argument."""
    gp = epowers(e2(lgamma), w + 1)
    cps = w if table_id is not None else w + 1
    beta = e2(lbeta)
    dens = []
    for i in range(reps):
        d = (beta[0] + np.zeros(Q, dtype=object), beta[1] + np.zeros(Q, dtype=object))
        for j in range(cps):
            d = eadd(d, escale(gp[j], res(lvars[i * cps + j][:Q])))
        if table_id is not None:
            d = eadd(d, escale(gp[w], res(table_id[:Q])))
        dens.append(d)
    d = (beta[0] + np.zeros(Q, dtype=object), beta[1] + np.zeros(Q, dtype=object))
    for j in range(w + 1):
        d = eadd(d, escale(gp[j], res(tables[j][:Q])))
    return dens + [d]


def lookup_term(lvars, table_id, tables, mult, A, B, reps, w, lbeta, lgamma, alphas, Q, T):
    """T + sum_i alpha_i (A_i den_i - 1) + alpha_reps (B den_table - mult); A as rows A_0.c0, A_0.c1, A_1.c0, ..."""
    dens = lookup_denominators(lvars, table_id, tables, reps, w, lbeta, lgamma, Q)
    for i in range(reps):
        t = emul((res(A[2 * i][:Q]), res(A[2 * i + 1][:Q])), dens[i])
        T = eadd(T, emul(e2(alphas[i]), ((t[0] - 1) % P, t[1])))
    t = emul((res(B[0][:Q]), res(B[1][:Q])), dens[reps])
    return eadd(T, emul(e2(alphas[reps]), ((t[0] - res(mult[:Q])) % P, t[1])))


def lookup_polys_ref(lvars, table_id, tables, mult, reps, w, n, lbeta, lgamma):
    """A_i = 1 / den_i, B = mult / den_table: ([reps][2][n], [2][n]) canonical words"""
    dens = lookup_denominators(lvars, table_id, tables, reps, w, lbeta, lgamma, n)
    A = np.stack([to_words(*einv(d)) for d in dens[:reps]])
    return A, to_words(*escale(einv(dens[reps]), res(mult[:n])))


# ---------------------------------------------------------------------------------------------- copy permutation
def copy_perm_term(vars, sigmas, stage2, non_res, chunk, log_n, log_lde, beta, gamma, alphas, first, count, T):
    """(T + alpha_L1 (z - 1) (x^n - 1) / (x - 1) + sum_j alpha_j (lhs_j prod (sigma_c beta + w_c + gamma) - rhs_j prod (k_c x beta
    + w_c + gamma))) / (x^n - 1) at the flat LDE indices first .. first + count.  Columns are indexed by the GLOBAL flat index
    ([cols][>= n << log_lde]); stage2 rows are z.c0, z.c1, p0.c0, p0.c1, ...; alphas = [alpha_L1, alpha_chunk0, ...]; T holds
    count points."""
    n, V = 1 << log_n, len(non_res)
    n_chunks = (V + chunk - 1) // chunk
    idx = np.arange(first, first + count)
    nxt = np.array([next_in_coset(int(I), log_n) for I in idx])
    x = lde_points(log_n, log_lde, first, count)
    xn1 = np.array([(coset_xn(log_n, log_lde, int(I) // n) - 1) % P for I in idx], dtype=object)
    beta, gamma = e2(beta), e2(gamma)

    def s2(row, at): return (res(np.asarray(stage2[row])[at]), res(np.asarray(stage2[row + 1])[at]))
    z = s2(0, idx)
    num = escale(emul(e2(alphas[0]), ((z[0] - 1) % P, z[1])), xn1 * inv((x - 1) % P) % P)
    for j in range(n_chunks):
        lhs = s2(2 + 2 * j, idx) if j + 1 < n_chunks else s2(0, nxt)
        rhs = z if j == 0 else s2(2 * j, idx)
        for c in range(j * chunk, min((j + 1) * chunk, V)):
            wv, sg, k = res(np.asarray(vars[c])[idx]), res(np.asarray(sigmas[c])[idx]), int(non_res[c]) % P
            lhs = emul(lhs, eadd(escale(beta, sg), ((wv + gamma[0]) % P, gamma[1])))
            rhs = emul(rhs, eadd(escale(beta, k * x % P), ((wv + gamma[0]) % P, gamma[1])))
        num = eadd(num, emul(e2(alphas[1 + j]), esub(lhs, rhs)))
    return escale(eadd(T, num), inv(xn1))
