"""CPU pins of the oracle functions that the large-size -m gpu operator tests lean on: the linear combination (oracle/pointwise.c,
our own definition) against Python integers, and the fixed-seed inputs of the grand-product scan tests above 2^18 rows, which
must have no zero denominator (the oracle inverts row by row and would turn one into a zero quietly)."""
import numpy as np
import pytest

import oracle as O
from gpu_util import rand_gl, scan_inputs

P = O.P


def _emul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


@pytest.mark.parametrize("n,n_base,n_ext,threads", [(1, 1, 0, 1), (1, 0, 1, 1), (5, 3, 2, 2), (64, 1, 4, 3), (257, 9, 7, 4)])
def test_linear_combination_matches_python_integers(n, n_base, n_ext, threads):
    rng = np.random.default_rng(n * 31 + n_base)
    base = rand_gl(rng, (max(n_base, 1), n), noncanonical=True)
    ext = rand_gl(rng, (max(n_ext, 1), 2, n), noncanonical=True)
    k = n_base + n_ext
    ch = rand_gl(rng, (k, 2), noncanonical=True)
    ch[0][0] = 0
    ch[-1][1] = P - 1
    srcs = [(base[i], None) for i in range(n_base)] + [(ext[i][0], ext[i][1]) for i in range(n_ext)]
    keep = [None if b is None else (a.copy(), b.copy()) for a, b in srcs]
    o0, o1 = O.linear_combination(srcs, ch, threads=threads)
    for i in range(n):
        acc = (0, 0)
        for j, (a, b) in enumerate(srcs):
            t = _emul((int(a[i]) % P, 0 if b is None else int(b[i]) % P), (int(ch[j][0]) % P, int(ch[j][1]) % P))
            acc = ((acc[0] + t[0]) % P, (acc[1] + t[1]) % P)
        assert (int(o0[i]), int(o1[i])) == acc, i
    assert o0.max() < P and o1.max() < P
    for (a, b), kp in zip(srcs, keep):                              # sources are read only
        if kp is not None:
            assert np.array_equal(a, kp[0]) and np.array_equal(b, kp[1])


@pytest.mark.parametrize("log_n", [18, 19, 20])
def test_scan_inputs_have_no_zero_denominator(log_n):
    """w + beta * sigma + gamma = 0 in F_p^2 needs sigma = -gamma_1 / beta_1 (the u component) and then w = -(beta_0 sigma + gamma_0):
    no cell of the fixed-seed columns may be that pair.  The oracle alone must also complete with z[0] = 1 and no zero in z (a
    zero numerator or denominator anywhere would zero every later row)."""
    from oracle import prover as OP
    from test_gpu_stage_ops import BETA, GAMMA
    variables, sigmas, non_res = scan_inputs(log_n)
    assert BETA[1] % P
    s_star = (-GAMMA[1] * O.inv(BETA[1])) % P
    w_star = (-(BETA[0] * s_star + GAMMA[0])) % P
    assert not np.any((O.canonical(sigmas) == np.uint64(s_star)) & (O.canonical(variables) == np.uint64(w_star)))
    z, partials = OP.copy_perm_stage2(variables, sigmas, non_res, log_n, 4, BETA, GAMMA, threads=4)
    assert z[0][0] == 1 and z[1][0] == 0 and partials.shape == (1, 2, 1 << log_n)
    assert not np.any((z[0] == 0) & (z[1] == 0)) and not np.any((partials[0][0] == 0) & (partials[0][1] == 0))
