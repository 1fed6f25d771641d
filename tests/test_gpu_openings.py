"""-m gpu parity: barycentric evaluation and DEEP quotient accumulation (through the C ABI) vs the CPU oracle
(whose DEEP point function is pinned by the golden proof, tests/test_oracle_fixture.py).  The second half reaches, operator by
operator, the paths only 2^19+-row or sharded proofs take: both variants of the linear combination, the multi-set DEEP kernel,
the range forms at first != 0 and the second trip of the barycentric final reduction."""
import numpy as np
import pytest

import oracle as O
from gpu_util import DevBuf, ctx, oracle_threads, rand_gl, P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log_n", [0, 1, 3, 8, 12, 15])
def test_barycentric_weights_and_eval_match_oracle(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    z = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
    w0, w1 = O.barycentric_weights(log_n, 7, z)
    d_w = DevBuf(nelems=2 * n)
    ctx().barycentric_weights(log_n, 7, z, d_w.ptr, d_w.ptr + 8 * n)
    got = d_w.get((2, n))
    assert np.array_equal(got[0], w0) and np.array_equal(got[1], w1)
    n_cols = 11
    cols = rand_gl(rng, (n_cols, n), noncanonical=True)
    d_c = DevBuf(cols)
    out = ctx().barycentric_eval_batch([d_c.ptr + 8 * n * c for c in range(n_cols)], log_n, d_w.ptr, d_w.ptr + 8 * n)
    for c in range(n_cols):
        assert (int(out[c][0]), int(out[c][1])) == O.barycentric_eval_base(cols[c], w0, w1), c
    # extension-valued polynomial stored as two columns: combine on the host as the ABI documents
    e0, e1 = out[0], out[1]
    comb = ((int(e0[0]) + 7 * int(e1[1])) % P, (int(e0[1]) + int(e1[0])) % P)
    if n > 1:
        assert comb == O.barycentric_eval_ext(cols[0], cols[1], w0, w1)
    d_w.free(); d_c.free()


def test_barycentric_equals_polynomial_evaluation_end_to_end():
    """trace -> (GPU) monomials -> LDE; evaluate every column at z from coset 0 of the LDE; compare with Horner."""
    log_n, log_lde, n_cols = 10, 2, 3
    n = 1 << log_n
    rng = np.random.default_rng(5)
    mono = rand_gl(rng, (n_cols, n))
    d_m, d_l = DevBuf(mono), DevBuf(nelems=n_cols * n << log_lde)
    ctx().lde_batch(d_m.ptr, d_l.ptr, log_n, n_cols, log_lde)
    z = (1234567, 7654321)
    d_w = DevBuf(nelems=2 * n)
    ctx().barycentric_weights(log_n, 7, z, d_w.ptr, d_w.ptr + 8 * n)
    out = ctx().barycentric_eval_batch([d_l.ptr + 8 * (n << log_lde) * c for c in range(n_cols)], log_n, d_w.ptr, d_w.ptr + 8 * n)
    for c in range(n_cols):
        acc, zp = (0, 0), (1, 0)
        for coef in mono[c]:
            acc = ((acc[0] + int(coef) * zp[0]) % P, (acc[1] + int(coef) * zp[1]) % P)
            zp = ((zp[0] * z[0] + 7 * zp[1] * z[1]) % P, (zp[0] * z[1] + zp[1] * z[0]) % P)
        assert (int(out[c][0]), int(out[c][1])) == acc
    d_m.free(); d_l.free(); d_w.free()


@pytest.mark.parametrize("log_n,log_lde,n_base,n_ext", [(4, 1, 1, 0), (6, 2, 5, 3), (10, 3, 40, 9), (13, 1, 3, 1)])
def test_deep_quotient_matches_oracle(log_n, log_lde, n_base, n_ext):
    N = 1 << (log_n + log_lde)
    rng = np.random.default_rng(log_n * 7 + n_ext)
    base_cols = rand_gl(rng, (n_base, N), noncanonical=True)
    ext_cols = rand_gl(rng, (max(n_ext, 1), 2, N))
    k = n_base + n_ext
    values = rand_gl(rng, (k, 2))
    challenges = rand_gl(rng, (k, 2))
    at = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
    dst = rand_gl(rng, (2, N), noncanonical=True)
    srcs = [(base_cols[i], None) for i in range(n_base)] + [(ext_cols[i][0], ext_cols[i][1]) for i in range(n_ext)]
    w0, w1 = dst[0].copy(), dst[1].copy()
    O.deep_quotient_accumulate(srcs, values, challenges, at, log_n, log_lde, w0, w1, threads=4)
    d_b, d_e, d_d = DevBuf(base_cols), DevBuf(ext_cols), DevBuf(dst)
    dsrc = [(d_b.ptr + 8 * N * i, None) for i in range(n_base)] + \
           [(d_e.ptr + 8 * N * (2 * i), d_e.ptr + 8 * N * (2 * i + 1)) for i in range(n_ext)]
    ctx().deep_quotient_accumulate(dsrc, values, challenges, at, log_n, log_lde, d_d.ptr, d_d.ptr + 8 * N, accumulate=True)
    got = d_d.get((2, N))
    assert np.array_equal(got[0], w0) and np.array_equal(got[1], w1)
    # overwrite mode == accumulate into zeros
    z0, z1 = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
    O.deep_quotient_accumulate(srcs, values, challenges, at, log_n, log_lde, z0, z1, threads=4)
    ctx().deep_quotient_accumulate(dsrc, values, challenges, at, log_n, log_lde, d_d.ptr, d_d.ptr + 8 * N, accumulate=False)
    got = d_d.get((2, N))
    assert np.array_equal(got[0], z0) and np.array_equal(got[1], z1)
    d_b.free(); d_e.free(); d_d.free()


@pytest.mark.timeout(240)
def test_deep_quotient_at_a_trace_domain_point_2p25():
    """The opening set of a public input: at = (omega_n^row, 0) over the 2^25-point LDE domain.  In one thread of this launch
    the running product of the four denominators has a 2-power order, so the inversion chain squares 2^48 (2^96 = -1):
    the borrow-without-carry branch of gl::mul_weak, taken in the middle of a counted loop.  (Its s_andn2_b64 writes SCC;
    with SCC missing from the asm clobbers the loop lost its exit test and ran 2^29 more trips.)  The single-set operator
    runs the multi-set kernel with one set: its running product is the same four norms in the same order, so this thread
    still takes that branch."""
    log_n, log_lde = 22, 3
    N = 1 << (log_n + log_lde)
    rng = np.random.default_rng(2225)
    col = rand_gl(rng, (1, N))
    values, challenges = rand_gl(rng, (1, 2)), rand_gl(rng, (1, 2))
    values[0][1] = 0
    om = pow(0x185629dcda58878c, 1 << (32 - log_n), P)
    at = (pow(om, 5, P), 0)
    dst = rand_gl(rng, (2, N))
    w0, w1 = dst[0].copy(), dst[1].copy()
    O.deep_quotient_accumulate([(col[0], None)], values, challenges, at, log_n, log_lde, w0, w1, threads=8)
    d_b, d_d = DevBuf(col), DevBuf(dst)
    ctx().deep_quotient_accumulate([(d_b.ptr, None)], values, challenges, at, log_n, log_lde, d_d.ptr, d_d.ptr + 8 * N,
                                   accumulate=True)
    got = d_d.get((2, N))
    assert np.array_equal(got[0], w0) and np.array_equal(got[1], w1)
    d_b.free(); d_d.free()


def test_deep_then_fri_is_low_degree():
    """Size-independent property: the DEEP combination of true openings of low-degree polynomials is itself a
    low-degree codeword, so bj_fri_prove accepts it (and rejects it if one opening value is wrong)."""
    import era_boojum_amd as E
    log_n, log_lde, n_cols, cap = 9, 2, 6, 4
    n, N = 1 << log_n, 1 << (log_n + log_lde)
    rng = np.random.default_rng(77)
    mono = rand_gl(rng, (n_cols, n))
    d_m, d_l = DevBuf(mono), DevBuf(nelems=n_cols * N)
    ctx().lde_batch(d_m.ptr, d_l.ptr, log_n, n_cols, log_lde)
    z = (424242, 171717)
    d_w = DevBuf(nelems=2 * n)
    ctx().barycentric_weights(log_n, 7, z, d_w.ptr, d_w.ptr + 8 * n)
    cols = [d_l.ptr + 8 * N * c for c in range(n_cols)]
    vals = ctx().barycentric_eval_batch(cols, log_n, d_w.ptr, d_w.ptr + 8 * n)
    chs = rand_gl(rng, (n_cols, 2))
    d_d = DevBuf(nelems=2 * N)
    _, _, sched, _ = E.fri_schedule(40, cap, 0, log_lde, log_n)
    for corrupt in (False, True):
        v = vals.copy()
        if corrupt:
            v[2][0] = (int(v[2][0]) + 1) % P
        ctx().deep_quotient_accumulate([(c, None) for c in cols], v, chs, z, log_n, log_lde, d_d.ptr, d_d.ptr + 8 * N,
                                       accumulate=False)
        t = E.Transcript()
        if corrupt:
            with pytest.raises(E.BoojumHipError):
                ctx().fri_prove(d_d.ptr, d_d.ptr + 8 * N, log_n, log_lde, sched, cap, t)
        else:
            ctx().fri_prove(d_d.ptr, d_d.ptr + 8 * N, log_n, log_lde, sched, cap, t).close()
    for b in (d_m, d_l, d_w, d_d):
        b.free()


# ---------------------------------------------------------------------------------------------------------------------------
# bj_linear_combination: linear_combination_kernel<1, 8> up to 2^18 entries (8 columns in flight + a remainder loop),
# <4, 1> above (four entries per lane)
# ---------------------------------------------------------------------------------------------------------------------------
# (base sources, F_p^2 sources) -> flattened columns 1, 7, 8, 8, 9, 16, 23
LC_SHAPES = [(1, 0), (3, 2), (8, 0), (0, 4), (1, 4), (6, 5), (9, 7)]
LC_CASES = [(n, nb, ne) for n in (1, 255, 256, 1000, 1 << 14) for nb, ne in LC_SHAPES] + \
           [(n, nb, ne) for n in (1 << 18, (1 << 18) + 1, 3 * (1 << 17) + 5, 1 << 19) for nb, ne in [(3, 2), (1, 4), (9, 7)]]


def _lc_challenges(rng, k):
    ch = rand_gl(rng, (k, 2))
    ch[0][0], ch[0][1] = np.uint64(0), np.uint64(P - 1)          # a zero component and p - 1
    if k > 1:
        ch[-1][1] = np.uint64(0)
    if k > 2:
        ch[1][0] = np.uint64(P - 1)
    if k > 3:
        ch[2][0], ch[2][1] = np.uint64(P + 5), np.uint64(0xFFFFFFFFFFFFFFFF)   # any representative is accepted
    return ch


@pytest.mark.parametrize("n,n_base,n_ext", LC_CASES)
def test_linear_combination_matches_oracle(n, n_base, n_ext):
    """Sources live at an odd offset inside a larger buffer (the way a rank passes its slice of the monomials), the outputs
    between guard cells: the result equals the oracle's, nothing outside [0, n) is written, the sources are left as they were."""
    rng = np.random.default_rng(n * 131 + 8 * n_base + n_ext)
    n_flat, off, guard = n_base + 2 * n_ext, 3, 5
    stride = off + n + 4
    host = rand_gl(rng, (n_flat, stride), noncanonical=True)
    cols = [host[c, off:off + n] for c in range(n_flat)]
    srcs = [(cols[i], None) for i in range(n_base)] + [(cols[n_base + 2 * i], cols[n_base + 2 * i + 1]) for i in range(n_ext)]
    ch = _lc_challenges(rng, n_base + n_ext)
    w0, w1 = O.linear_combination(srcs, ch, threads=oracle_threads(16))
    d_s = DevBuf(host)
    ptr = [d_s.ptr + 8 * (c * stride + off) for c in range(n_flat)]
    dsrc = [(ptr[i], None) for i in range(n_base)] + [(ptr[n_base + 2 * i], ptr[n_base + 2 * i + 1]) for i in range(n_ext)]
    fill = np.full((2, n + 2 * guard), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d_o = DevBuf(fill)
    ctx().linear_combination(dsrc, ch, n, d_o.ptr + 8 * guard, d_o.ptr + 8 * (n + 3 * guard))
    got = d_o.get((2, n + 2 * guard))
    assert np.array_equal(got[0][guard:guard + n], w0) and np.array_equal(got[1][guard:guard + n], w1)
    assert np.array_equal(got[:, :guard], fill[:, :guard]) and np.array_equal(got[:, guard + n:], fill[:, guard + n:])
    assert np.array_equal(d_s.get((n_flat, stride)), host)
    d_s.free(); d_o.free()


# ---------------------------------------------------------------------------------------------------------------------------
# bj_deep_quotient_accumulate_sets / _range: the multi-set kernel and both kernels on a rank's slice of the LDE domain
# ---------------------------------------------------------------------------------------------------------------------------
class _DeepSets:
    """Three opening sets shaped like the prover's: a wide one at a random z (base and F_p^2 sources), a narrow one at z * omega,
    a narrow one at 0.  Host columns for the oracle, device columns for the operators."""

    def __init__(self, log_n, log_lde, seed, wide=(6, 3)):
        self.log_n, self.log_lde, self.N = log_n, log_lde, 1 << (log_n + log_lde)
        rng = np.random.default_rng(seed)
        z = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
        om = O.omega(log_n)
        shapes = [(wide, z), ((0, 2), (z[0] * om % P, z[1] * om % P)), ((1, 1), (0, 0))]
        self.host, self.bufs, self.sets, self.dsets = [], [], [], []
        for (nb, ne), at in shapes:
            cols = rand_gl(rng, (nb + 2 * ne, self.N), noncanonical=True)
            d = DevBuf(cols)
            self.host.append(cols); self.bufs.append(d)
            vals, chs = rand_gl(rng, (nb + ne, 2)), rand_gl(rng, (nb + ne, 2))
            pair = lambda f, i: (f(i), None) if i < nb else (f(nb + 2 * (i - nb)), f(nb + 2 * (i - nb) + 1))
            self.sets.append(([pair(lambda c: cols[c], i) for i in range(nb + ne)], vals, chs, at))
            self.dsets.append(([pair(lambda c: d.ptr + 8 * self.N * c, i) for i in range(nb + ne)], vals, chs, at))
        self.rng = rng

    def oracle(self, n_sets, dst, first=0, count=None):
        """dst [2][count] (any representatives) + the first n_sets sets on [first, first + count), set by set."""
        count = self.N - first if count is None else count
        w0, w1 = dst[0].copy(), dst[1].copy()
        for srcs, vals, chs, at in self.sets[:n_sets]:
            sl = [(a[first:first + count], None if b is None else b[first:first + count]) for a, b in srcs]
            O.deep_quotient_accumulate_range(sl, vals, chs, at, self.log_n, self.log_lde, first, w0, w1, threads=oracle_threads(16))
        return np.stack([w0, w1])

    def device(self, n_sets, first=0):
        """The first n_sets device sets with every source pointer moved to the entry of LDE index `first`."""
        return [([(a + 8 * first, None if b is None else b + 8 * first) for a, b in srcs], vals, chs, at)
                for srcs, vals, chs, at in self.dsets[:n_sets]]

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("log_n,log_lde", [(4, 1), (7, 2), (10, 3), (18, 2)])
def test_deep_multi_set_matches_the_oracle_set_by_set(log_n, log_lde):
    """N = 32, 512 (below one workgroup's 1024 points), 2^13 and 2^20; 1, 2 and 3 sets; overwrite and accumulate (onto a
    destination with non-canonical words); and the same sets through single-set range calls give the same buffer."""
    S = _DeepSets(log_n, log_lde, seed=1000 + log_n)
    N = S.N
    dst = rand_gl(S.rng, (2, N), noncanonical=True)
    zero = np.zeros((2, N), dtype=np.uint64)
    d_d, d_e = DevBuf(dst), DevBuf(dst)
    for n_sets in (1, 2, 3):
        for accumulate in (0, 1):
            ctx().h2d(d_d.ptr, dst)
            ctx().deep_quotient_accumulate_sets(S.device(n_sets), log_n, log_lde, 0, N, d_d.ptr, d_d.ptr + 8 * N, accumulate)
            got = d_d.get((2, N))
            assert np.array_equal(got, S.oracle(n_sets, dst if accumulate else zero)), (n_sets, accumulate)
            ctx().h2d(d_e.ptr, dst)
            for t, (srcs, vals, chs, at) in enumerate(S.device(n_sets)):
                ctx().deep_quotient_accumulate_range(srcs, vals, chs, at, log_n, log_lde, 0, N, d_e.ptr, d_e.ptr + 8 * N,
                                                     accumulate or t > 0)
            assert np.array_equal(d_e.get((2, N)), got), (n_sets, accumulate)
    d_d.free(); d_e.free(); S.free()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_deep_range_forms_rank_by_rank_give_the_full_domain_result(world):
    """Every rank's slice [r N / world, (r + 1) N / world) computed on its own, through the single-set and through the multi-set
    entry, with pointers that address the slice: the slices side by side are the oracle's full-domain result."""
    log_n, log_lde = 9, 3
    S = _DeepSets(log_n, log_lde, seed=2000 + world, wide=(3, 2))
    N = S.N
    per = N // world
    dst = rand_gl(S.rng, (2, N), noncanonical=True)
    want = S.oracle(3, dst)
    d_a, d_b = DevBuf(dst), DevBuf(dst)
    for r in range(world):
        first = r * per
        sets = S.device(3, first)
        ctx().deep_quotient_accumulate_sets(sets, log_n, log_lde, first, per, d_a.ptr + 8 * first, d_a.ptr + 8 * (N + first), 1)
        for srcs, vals, chs, at in sets:
            ctx().deep_quotient_accumulate_range(srcs, vals, chs, at, log_n, log_lde, first, per, d_b.ptr + 8 * first,
                                                 d_b.ptr + 8 * (N + first), 1)
    assert np.array_equal(d_a.get((2, N)), want)
    assert np.array_equal(d_b.get((2, N)), want)
    d_a.free(); d_b.free(); S.free()


@pytest.mark.parametrize("accumulate", [0, 1])
def test_deep_range_forms_at_an_odd_first_and_a_ragged_count(accumulate):
    """first = 1001 (odd: x_I takes the negated twiddle first), count = 1531 (one full workgroup of 1024 points and a clamped
    tail): the range is the oracle's, the destination outside it is untouched."""
    log_n, log_lde, first, count = 9, 3, 1001, 1531
    S = _DeepSets(log_n, log_lde, seed=3000 + accumulate, wide=(3, 2))
    N = S.N
    dst = rand_gl(S.rng, (2, N), noncanonical=True)
    inside = dst[:, first:first + count] if accumulate else np.zeros((2, count), dtype=np.uint64)
    want = dst.copy()
    want[:, first:first + count] = S.oracle(3, inside, first, count)
    sets = S.device(3, first)
    d_a, d_b = DevBuf(dst), DevBuf(dst)
    ctx().deep_quotient_accumulate_sets(sets, log_n, log_lde, first, count, d_a.ptr + 8 * first, d_a.ptr + 8 * (N + first), accumulate)
    for t, (srcs, vals, chs, at) in enumerate(sets):
        ctx().deep_quotient_accumulate_range(srcs, vals, chs, at, log_n, log_lde, first, count, d_b.ptr + 8 * first,
                                             d_b.ptr + 8 * (N + first), accumulate or t > 0)
    assert np.array_equal(d_a.get((2, N)), want)
    assert np.array_equal(d_b.get((2, N)), want)
    d_a.free(); d_b.free(); S.free()


def test_opening_operators_report_bad_arguments():
    import era_boojum_amd as E
    log_n, log_lde = 4, 1
    N = 1 << (log_n + log_lde)
    d = DevBuf(np.zeros(4 * N, dtype=np.uint64))
    src, one = [(d.ptr, None)], [(1, 0)]
    st = (src, one, one, (5, 6))
    C = ctx()
    dst = (d.ptr + 8 * 2 * N, d.ptr + 8 * 3 * N)
    with pytest.raises(E.BoojumHipError, match="null"):
        C.linear_combination(src, one, N, None, dst[1])
    with pytest.raises(E.BoojumHipError, match="null source"):
        C.linear_combination([(None, None)], one, N, *dst)
    with pytest.raises(E.BoojumHipError, match="n = 0"):
        C.linear_combination(src, one, 0, *dst)
    with pytest.raises(E.BoojumHipError, match="bj_linear_combination"):
        C.linear_combination([], [], N, *dst)
    with pytest.raises(E.BoojumHipError, match="null"):
        C.deep_quotient_accumulate_range(src, one, one, (5, 6), log_n, log_lde, 0, N, dst[0], None)
    with pytest.raises(E.BoojumHipError, match="null source"):
        C.deep_quotient_accumulate_range([(None, None)], one, one, (5, 6), log_n, log_lde, 0, N, *dst)
    with pytest.raises(E.BoojumHipError, match="passes the"):
        C.deep_quotient_accumulate_range(src, one, one, (5, 6), log_n, log_lde, N - 7, 8, *dst)
    with pytest.raises(E.BoojumHipError, match="passes the"):
        C.deep_quotient_accumulate_range(src, one, one, (5, 6), log_n, log_lde, 2 ** 64 - 4, 8, *dst)     # first + count wraps
    with pytest.raises(E.BoojumHipError, match="empty"):
        C.deep_quotient_accumulate_range(src, one, one, (5, 6), log_n, log_lde, 3, 0, *dst)
    with pytest.raises(E.BoojumHipError, match="0 opening sets"):
        C.deep_quotient_accumulate_sets([], log_n, log_lde, 0, N, *dst)
    with pytest.raises(E.BoojumHipError, match="4 opening sets"):
        C.deep_quotient_accumulate_sets([st] * 4, log_n, log_lde, 0, N, *dst)
    with pytest.raises(E.BoojumHipError, match="passes the"):
        C.deep_quotient_accumulate_sets([st], log_n, log_lde, 1, N, *dst)
    with pytest.raises(E.BoojumHipError, match="empty"):
        C.deep_quotient_accumulate_sets([st], log_n, log_lde, 0, 0, *dst)
    with pytest.raises(E.BoojumHipError, match="null"):
        C.deep_quotient_accumulate_sets([st], log_n, log_lde, 0, N, None, dst[1])
    with pytest.raises(E.BoojumHipError, match="null source 0 of set 1"):
        C.deep_quotient_accumulate_sets([st, ([(None, None)], one, one, (5, 6))], log_n, log_lde, 0, N, *dst)
    assert not d.get().any()                            # nothing was launched
    C.deep_quotient_accumulate_sets([st] * 3, log_n, log_lde, 0, N, *dst)      # and the context still works: 3 sets are taken
    d.free()


def test_barycentric_evaluation_at_2p22_rows():
    """2^22 rows are 512 partial blocks per column: barycentric_final_kernel's strided loop takes its second trip (the other sizes
    here stop at 4 blocks).  Nine columns: one full group of eight and a remainder of one in the partial kernel."""
    log_n, n_cols = 22, 9
    n = 1 << log_n
    rng = np.random.default_rng(2222)
    z = (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))
    w0, w1 = O.barycentric_weights(log_n, 7, z)
    d_w = DevBuf(nelems=2 * n)
    ctx().barycentric_weights(log_n, 7, z, d_w.ptr, d_w.ptr + 8 * n)
    got = d_w.get((2, n))
    assert np.array_equal(got[0], w0) and np.array_equal(got[1], w1)
    cols = rand_gl(rng, (n_cols, n), noncanonical=True)
    d_c = DevBuf(cols)
    out = ctx().barycentric_eval_batch([d_c.ptr + 8 * n * c for c in range(n_cols)], log_n, d_w.ptr, d_w.ptr + 8 * n)
    for c in range(n_cols):
        assert (int(out[c][0]), int(out[c][1])) == O.barycentric_eval_base(cols[c], w0, w1), c
    d_w.free(); d_c.free()
