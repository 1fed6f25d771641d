"""-m gpu: the three kernel families that otherwise run only inside bj_prove, each through its own entry point and against its
one-line definition, word for word.

  * eval_monomials_at_kernel (csrc/openings.hip) through Context.eval_monomials_at: out[j][c] = sum_i mono_c[i] * x_j^i at the
    point of a leaf of the LDE domain.  Horner in Python integers up to 2^10 coefficients, the indexed leaf of oracle.lde_batch
    above (the two agree at 2^10); every split of the exponent walk: fewer coefficients than lanes, U = 1, the tail loop, U = 8,
    U = 2048 with K = 1, the outer Horner loop (K = 2, 4, 8) and the tiled layout at 2^22.
  * sponge_leaves_absorb (csrc/sponge_tree.h: poseidon2_ / poseidon1_leaves_absorb_kernel) through Context.merkle_leaves_absorb:
    the digests of a leaf hashing split into column groups against the oracle's leaf hash and layer 0 of merkle_tree_build, and
    with first = 0, last = 1 all twelve state words from the test: the rare branches of gl::mul_weak inside these two kernels.
  * byte_pow (csrc/byte_tree.h: blake2s_ / keccak_pow_kernel) through Context.pow_search: the smallest accepted nonce of a
    window, or ~0, against oracle.prover._pow_first_words (hashlib / oracle/keccak.py) over the same window.
"""
import functools
import json
import os

import numpy as np
import pytest

import era_boojum_amd as E
import oracle as O
from gpu_util import DevBuf, ctx, oracle_threads, rand_gl
from oracle import prover as OP

import poseidon1_layer as PL
import poseidon_rare as PR

pytestmark = pytest.mark.gpu

P = E.P
M64 = (1 << 64) - 1
GUARD = 16
SENTINEL = 0xA5A5A5A5DEADBEEF
HASHER_POSEIDON2, HASHER_BLAKE2S, HASHER_KECCAK256, HASHER_POSEIDON = 1, 2, 3, 4
POW_BLAKE2S256, POW_KECCAK256 = 1, 2


# ------------------------------------------------------------------------------------------------ evaluation kernel
def leaf_point(leaf, log_full):
    """x of a leaf: 7 * omega^bitrev(leaf) in the 2^log_full-point LDE domain."""
    return 7 * pow(O.omega(log_full), O.bitrev(leaf, log_full), P) % P


def horner(coeffs, x):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % P
    return acc


def horner_rows(cols, log_full, leaves):
    """[leaf][column] from the definition; cols: (n_cols, n) of any u64 words."""
    ints = [[int(v) for v in col] for col in cols]
    return np.array([[horner(col, leaf_point(int(I), log_full)) for col in ints] for I in leaves], dtype=np.uint64)


def quarter_noncanonical(rng, shape):
    """A quarter of the words in [p, 2^64), the rest random residues."""
    a = rand_gl(rng, shape)
    hi = np.uint64(P) + rng.integers(0, M64 - P + 1, size=shape, dtype=np.uint64)
    return np.where(rng.random(size=shape) < 0.25, hi, a)


def special_columns(n):
    """The accumulator's worst case and the ends of the walk: all 2^64 - 1, all p - 1, only the last coefficient, only coefficient 0."""
    s = np.zeros((4, n), dtype=np.uint64)
    s[0], s[1] = M64, P - 1
    s[2, n - 1] = 0x123456789ABCDEF
    s[3, 0] = M64 - 1
    return s


def leaf_set(rng, n, log_lde, n_idx):
    """Leaf 0 (x = 7), N - 1, a repeated leaf, adjacent leaves, one leaf of every coset, then random ones up to n_idx."""
    N = n << log_lde
    if n_idx == 1:
        return [N - 1]
    fixed = [0, N - 1, 0, N // 2, min(N // 2 + 1, N - 1), max(N - 2, 0)] + [c * n + int(rng.integers(0, n)) for c in range(1 << log_lde)]
    more = [int(v) for v in rng.integers(0, N, size=max(0, n_idx - len(fixed)))]
    return (fixed + more)[:max(n_idx, len(fixed))]


def run_eval(mono, log_n, log_lde, idx, stride_pad=0, tiled=False, first_leaf=0, d_mono=None):
    """mono: (n_cols, n).  Uploads it with `stride_pad` gap words per column and guard words behind, evaluates at idx into an output block
    between guard words, checks that gaps, guards and coefficients are what they were.  Returns (n_idx, n_cols)."""
    n_cols, n = mono.shape
    stride = n + stride_pad
    idx = np.array(idx, dtype=np.uint64)
    out_host = np.full(2 * GUARD + idx.size * n_cols, SENTINEL, dtype=np.uint64)
    d_idx, d_out = DevBuf(idx), DevBuf(out_host)
    buf = None
    if d_mono is None:
        buf = np.full(n_cols * stride + GUARD, SENTINEL, dtype=np.uint64)
        buf[:n_cols * stride].reshape(n_cols, stride)[:, :n] = mono
        d_buf = DevBuf(buf)
        d_mono = d_buf.ptr
    try:
        ctx().eval_monomials_at(d_mono, stride, n_cols, log_n, log_lde, d_idx.ptr, idx.size, d_out.ptr + 8 * GUARD, tiled=tiled,
                                first_leaf=first_leaf)
        got = d_out.get()
        assert np.all(got[:GUARD] == SENTINEL) and np.all(got[-GUARD:] == SENTINEL), "guard words around the output"
        if buf is not None:
            assert np.array_equal(d_buf.get(), buf), "the monomials, their gaps or the guard behind them were written"
        assert np.array_equal(d_idx.get(), idx)
        return got[GUARD:-GUARD].reshape(idx.size, n_cols)
    finally:
        d_idx.free()
        d_out.free()
        if buf is not None:
            d_buf.free()


# log_n, log_lde, n_cols, stride_pad, n_idx: fewer coefficients than lanes (0, 1, 5, 7), U = 1 (8), the tail loop U < 8 (9, 10)
SMALL = [(0, 3, 3, 1, 100), (1, 3, 3, 1, 100), (5, 3, 3, 1, 100), (7, 3, 3, 64, 100), (8, 3, 3, 1, 100), (9, 3, 3, 1, 100),
         (10, 3, 3, 64, 100), (10, 1, 40, 1, 14), (8, 2, 40, 64, 1), (9, 1, 1, 0, 1), (0, 1, 1, 0, 2), (7, 1, 1, 1, 100)]


@pytest.mark.parametrize("log_n,log_lde,n_cols,stride_pad,n_idx", SMALL)
def test_eval_monomials_from_the_definition(log_n, log_lde, n_cols, stride_pad, n_idx):
    """Up to 2^10 coefficients against Horner at x = 7 * omega^bitrev(leaf) in Python integers: a quarter of the words in
    [p, 2^64), and the four special columns in place of the first ones where there is room."""
    rng = np.random.default_rng(5000 + 100 * log_n + n_cols + n_idx)
    n = 1 << log_n
    mono = quarter_noncanonical(rng, (n_cols, n))
    if n_cols >= 40:
        mono[:4] = special_columns(n)
    elif n_cols == 3:
        mono[:2] = special_columns(n)[[0, 2]]
    leaves = leaf_set(rng, n, log_lde, n_idx)
    got = run_eval(mono, log_n, log_lde, leaves, stride_pad)
    assert np.array_equal(got, horner_rows(mono, log_n + log_lde, leaves))


def test_eval_monomials_special_columns_small():
    """All 2^64 - 1, all p - 1, only the last coefficient, only coefficient 0 at every small size, one launch each."""
    rng = np.random.default_rng(5100)
    for log_n in (0, 1, 5, 7, 8, 9, 10):
        n = 1 << log_n
        mono = special_columns(n)
        leaves = leaf_set(rng, n, 2, 12)
        assert np.array_equal(run_eval(mono, log_n, 2, leaves, 1), horner_rows(mono, log_n + 2, leaves)), log_n


def test_eval_monomials_of_a_shard():
    """first_leaf != 0 as a rank of a sharded domain passes it: cosets 2 to 3 of 8 with local indices give the values of the same
    leaves addressed from 0, and those of the definition."""
    log_n, log_lde = 8, 3
    n = 1 << log_n
    rng = np.random.default_rng(5200)
    mono = quarter_noncanonical(rng, (3, n))
    local = [0, 2 * n - 1, n, n - 1, 5, 5, 6] + [int(v) for v in rng.integers(0, 2 * n, size=40)]
    sharded = run_eval(mono, log_n, log_lde, local, 1, first_leaf=2 * n)
    whole = run_eval(mono, log_n, log_lde, [2 * n + i for i in local], 1)
    assert np.array_equal(sharded, whole)
    assert np.array_equal(whole, horner_rows(mono, log_n + log_lde, [2 * n + i for i in local]))


@functools.lru_cache(maxsize=2)
def _large(log_n):
    """Monomials (n_cols, n) and their oracle LDE at log_lde = 1.  2^11 and 2^19: the four special columns, a column with a quarter
    of its words in [p, 2^64) and a random one; from 2^20: the all-(2^64 - 1) column and the quarter column."""
    rng = np.random.default_rng(6000 + log_n)
    n = 1 << log_n
    if log_n < 20:
        mono = np.concatenate([special_columns(n), quarter_noncanonical(rng, (1, n)), rand_gl(rng, (1, n))])
    else:
        mono = np.concatenate([special_columns(n)[:1], quarter_noncanonical(rng, (1, n))])
    lde = O.lde_batch(mono, 1, threads=oracle_threads())
    mono.setflags(write=False)
    lde.setflags(write=False)
    return mono, lde


def _oracle_rows(lde, leaves):
    n = lde.shape[2]
    return np.array([[lde[c, I // n, I % n] for c in range(lde.shape[0])] for I in leaves], dtype=np.uint64)


def test_oracle_lde_is_the_definition_at_2p10():
    """The two references on their overlap: the indexed leaves of oracle.lde_batch are Horner's values, non-canonical words included."""
    rng = np.random.default_rng(5300)
    mono = np.concatenate([special_columns(1 << 10), quarter_noncanonical(rng, (2, 1 << 10))])
    leaves = leaf_set(rng, 1 << 10, 1, 20)
    want = horner_rows(mono, 11, leaves)
    assert np.array_equal(_oracle_rows(O.lde_batch(mono, 1), leaves), want)
    assert np.array_equal(run_eval(mono, 10, 1, leaves, 1), want)


# U = 8 (11), U = 2048 with K = 1 (19), the outer Horner loop K = 2, 4 (20, 21) and K = 8 on natural-order 2^22 columns
@pytest.mark.parametrize("log_n,stride_pad,n_idx", [(11, 1, 100), (19, 64, 100), (19, 1, 1), (20, 1, 100), (20, 64, 1), (21, 64, 100),
                                                    (22, 64, 100)])
def test_eval_monomials_against_the_oracle_lde(log_n, stride_pad, n_idx):
    mono, lde = _large(log_n)
    rng = np.random.default_rng(6100 + log_n + n_idx)
    leaves = leaf_set(rng, 1 << log_n, 1, n_idx)
    got = run_eval(mono, log_n, 1, leaves, stride_pad)
    assert np.array_equal(got, _oracle_rows(lde, leaves))


def test_eval_monomials_tiled_at_2p22():
    """The tiled walk on columns laid out by bj_tiled_permute_batch: the values of the natural walk and of the oracle on the same
    leaves; n_idx = 1 as well."""
    log_n, pad = 22, 64
    mono, lde = _large(log_n)
    n_cols, n = mono.shape
    stride = n + pad
    rng = np.random.default_rng(6200)
    leaves = leaf_set(rng, n, 1, 100)
    buf = np.full((n_cols, stride), SENTINEL, dtype=np.uint64)
    buf[:, :n] = mono
    d_nat, d_til = DevBuf(buf), DevBuf(np.full(n_cols * stride + GUARD, SENTINEL, dtype=np.uint64))
    try:
        ctx().tiled_permute_batch(d_nat.ptr, d_til.ptr, log_n, n_cols, True, col_stride=stride)
        before = d_til.get()
        assert not np.array_equal(before[stride:stride + n], mono[1])  # the random column lies otherwise: the natural walk would misread it
        assert np.array_equal(np.sort(before[stride:stride + n]), np.sort(mono[1]))
        tiled = run_eval(mono, log_n, 1, leaves, pad, tiled=True, d_mono=d_til.ptr)
        natural = run_eval(mono, log_n, 1, leaves, pad, d_mono=d_nat.ptr)
        assert np.array_equal(tiled, natural)
        assert np.array_equal(tiled, _oracle_rows(lde, leaves))
        assert np.array_equal(run_eval(mono, log_n, 1, [leaves[1]], pad, tiled=True, d_mono=d_til.ptr), _oracle_rows(lde, [leaves[1]]))
        assert np.array_equal(d_til.get(), before)
    finally:
        d_nat.free()
        d_til.free()


# ------------------------------------------------------------------------------------------------ grouped absorption
EDGE_WORDS = [0, 1, P - 1, P, M64]
PLANS = [(1, (1,)), (7, (7,)), (8, (8,)), (9, (8, 1)), (16, (8, 8)), (16, (16,)), (29, (8, 8, 13)), (29, (16, 13)), (29, (24, 5)),
         (29, (29,)), (93, (8,) * 11 + (5,)), (93, (40, 48, 5))]
LEAF_COUNTS = [1, 63, 64, 65, 257, 1000]


def _leaf_hashes(hasher, rows):
    """The oracle's leaf hash of every row: oracle.hash_leaf for Poseidon2, tests/poseidon1_layer.py for v1."""
    if hasher == HASHER_POSEIDON2:
        return np.stack([O.hash_leaf(np.ascontiguousarray(r)) for r in rows])
    return PL.poseidon1_layer()._leaves(np.ascontiguousarray(rows))


def _absorb_columns(rng, n_cols, num_leaves, stride):
    """Random columns with non-canonical words, edge words on lone lanes and, where there are that many leaves, on whole waves."""
    buf = rand_gl(rng, (n_cols, stride), noncanonical=True)
    for k, w in enumerate(EDGE_WORDS):
        buf[(3 * k) % n_cols, (11 * k + 5) % num_leaves] = w           # lone lanes
        if num_leaves >= 64 * (k + 2):
            buf[:, 64 * (k + 1):64 * (k + 2)] = w                       # wave k + 1: every word of every leaf
    return buf


def _run_groups(hasher, buf, num_leaves, groups):
    """One leaf hashing over the column groups.  Capacity starts as garbage, digests as the sentinel; both lie before guard words."""
    c = ctx()
    n_cols, stride = buf.shape
    rng = np.random.default_rng(n_cols * 1000 + num_leaves)
    cap_host = rng.integers(0, 1 << 63, size=4 * num_leaves + GUARD, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    dig_host = np.full(4 * num_leaves + GUARD, SENTINEL, dtype=np.uint64)
    d_cols, d_cap, d_dig = DevBuf(buf), DevBuf(cap_host), DevBuf(dig_host)
    try:
        at = 0
        for g, width in enumerate(groups):
            first, last = g == 0, g == len(groups) - 1
            c.merkle_leaves_absorb(d_cols.ptr + 8 * at * stride, stride, width, num_leaves, d_cap.ptr, d_dig.ptr, first, last)
            at += width
            cap = d_cap.get()
            assert np.array_equal(cap[4 * num_leaves:], cap_host[4 * num_leaves:]), "guard words behind the capacity words"
            if not last:
                assert np.array_equal(d_dig.get(), dig_host), "a group that is not the last wrote digests"
            elif len(groups) == 1:
                assert np.array_equal(cap, cap_host), "a single group wrote capacity words"
        assert at == n_cols
        dig = d_dig.get()
        assert np.all(dig[4 * num_leaves:] == SENTINEL), "guard words behind the digests"
        assert np.array_equal(d_cols.get(buf.shape), buf)
        return dig[:4 * num_leaves].reshape(num_leaves, 4)
    finally:
        for b in (d_cols, d_cap, d_dig):
            b.free()


@functools.lru_cache(maxsize=None)
def _absorb_reference(hasher, n_cols, num_leaves):
    """(columns with their gap, oracle digests, layer 0 of merkle_tree_build over the same columns), shared by the plans of a width."""
    rng = np.random.default_rng(7000 + 10 * n_cols + hasher)
    pow2 = 1 << (num_leaves - 1).bit_length()
    stride = pow2 + 3
    buf = _absorb_columns(rng, n_cols, num_leaves, stride)
    want = _leaf_hashes(hasher, np.ascontiguousarray(buf[:, :num_leaves].T))
    d_cols, d_tree = DevBuf(buf), DevBuf(nelems=4 * pow2)
    try:
        ctx().merkle_tree_build(d_cols.ptr, stride, n_cols, pow2, pow2, d_tree.ptr)      # cap = leaves: the tree is its layer 0
        layer0 = d_tree.get((pow2, 4))[:num_leaves]
    finally:
        d_cols.free()
        d_tree.free()
    for a in (buf, want, layer0):
        a.setflags(write=False)
    return buf, want, layer0


@pytest.fixture
def hasher(request):
    ctx().set_tree_hasher(request.param)
    yield request.param
    ctx().set_tree_hasher(HASHER_POSEIDON2)


both_hashers = pytest.mark.parametrize("hasher", [HASHER_POSEIDON2, HASHER_POSEIDON], indirect=True, ids=["poseidon2", "poseidon"])


@both_hashers
@pytest.mark.parametrize("n_cols,groups", PLANS, ids=["%d_as_%s" % (n, "_".join(map(str, g)) if len(g) < 6 else "8x11_5") for n, g in PLANS])
def test_grouped_absorption_is_the_leaf_hash(hasher, n_cols, groups):
    """Every group plan at 1, 63, 64, 65, 257 and 1000 leaves under a column stride above the leaf count: the digests are the
    oracle's leaf hashes and layer 0 of merkle_tree_build; the first group ignores what the capacity buffer held, a group that
    is not the last leaves the digests alone, guard words stay."""
    assert sum(groups) == n_cols
    for num_leaves in LEAF_COUNTS:
        buf, want, layer0 = _absorb_reference(hasher, n_cols, num_leaves)
        got = _run_groups(hasher, buf, num_leaves, groups)
        assert np.array_equal(got, want), num_leaves
        assert np.array_equal(got, layer0), num_leaves


WAVE = 64


def _spread(cases, fill):
    """Wave c holds case c on one lane among random rows, wave len(cases) + c holds it on every lane (as the rare-product tests)."""
    cases = np.asarray(cases, dtype=np.uint64)
    k = len(cases)
    rows = fill(2 * k * WAVE)
    lone = np.array([WAVE * c + (7 * c + 3) % WAVE for c in range(k)])
    whole = np.array([WAVE * (k + c) for c in range(k)])
    rows[lone] = cases
    for c in range(k):
        rows[whole[c]:whole[c] + WAVE] = cases[c]
    return rows, lone, whole


def _rare_states(hasher, cls, rng):
    """Twelve-word states whose permutation takes a rare branch of gl::mul_weak: for v1 the constructions of tests/poseidon_rare.py
    (a fixture value at the S-box input of a chosen round), for Poseidon2 the first round's S-box inputs solved through the
    external matrix (as tests/test_gpu_poseidon2.py builds them) for the fixture values, 2^48 and the rare-product vectors."""
    states = []
    if hasher == HASHER_POSEIDON:
        for ent in PR.entries("weak", cls):
            for r in (0, 1, 3, 4, 15, 25, 26, 29):
                for words in (([r % 12], range(12)) if PR.is_full(r) else ([0],)):
                    st = PR.v1_construct(r, list(words), ent["x"], rng)
                    assert all(PR.v1_forward(st)[1][r][k] == ent["x"] for k in words)
                    states.append(st)
        return states
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gl_mul_rare.json")) as f:
        rare = [v["a"] % P for v in json.load(f)["vectors"] if v["class"] == cls]
    xs = sorted({e["x"] for e in PR.entries("weak", cls)}) + rare[:6] + ([1 << 48, (3 << 48) % P] if cls == 1 else [])
    for x in xs:
        for words in [range(12)] + [[k] for k in (0, 5, 8, 11)]:
            target = [int(v) for v in rng.integers(0, P, size=12, dtype=np.uint64)]
            for k in words:
                target[k] = x
            st = PR.solve_mod_p(PR.EXT, [(t - rc) % P for t, rc in zip(target, PR.RC[0])])
            assert [(sum(PR.EXT[i][j] * st[j] for j in range(12)) + PR.RC[0][i]) % P for i in range(12)] == target
            states.append(st)
    return states


@both_hashers
@pytest.mark.parametrize("cls", [1, 3])
def test_absorb_kernels_at_rare_sbox_products(hasher, cls):
    """first = 0, last = 1 on eight columns and caller-written capacity words: the kernel permutes the twelve words the test chose.
    Every constructed state on a lone lane of a random wave and on a whole wave; expected are the first four words of the oracle's
    permutation.  The same call with first = 1 must not read the capacity words: the hash of the eight rate words."""
    rng = np.random.default_rng(7500 + 10 * hasher + cls)
    cases = _rare_states(hasher, cls, rng)
    assert cases
    rows, lone, whole = _spread(cases, lambda k: rand_gl(rng, (k, 12), noncanonical=True))
    num_leaves = rows.shape[0]
    stride = num_leaves + 5
    cols = np.full((8, stride), SENTINEL, dtype=np.uint64)
    cols[:, :num_leaves] = rows[:, :8].T
    cap_host = np.concatenate([np.ascontiguousarray(rows[:, 8:].T).reshape(-1), np.full(GUARD, SENTINEL, dtype=np.uint64)])
    d_cols, d_cap, d_dig = DevBuf(cols), DevBuf(cap_host), DevBuf(np.full(4 * num_leaves + GUARD, SENTINEL, dtype=np.uint64))
    try:
        ctx().merkle_leaves_absorb(d_cols.ptr, stride, 8, num_leaves, d_cap.ptr, d_dig.ptr, False, True)
        got = d_dig.get()
        assert np.all(got[4 * num_leaves:] == SENTINEL) and np.array_equal(d_cap.get(), cap_host)
        got = got[:4 * num_leaves].reshape(num_leaves, 4)
        permute = O.poseidon2_permutation if hasher == HASHER_POSEIDON2 else O.poseidon_permutation
        for c, st in enumerate(cases):
            want = permute(np.array(st, dtype=np.uint64))[:4]
            assert np.array_equal(got[lone[c]], want), ("lone lane", c)
            assert np.array_equal(got[whole[c]:whole[c] + WAVE], np.tile(want, (WAVE, 1))), ("whole wave", c)
        assert np.array_equal(got, np.stack([permute(r) for r in rows])[:, :4])
        ctx().merkle_leaves_absorb(d_cols.ptr, stride, 8, num_leaves, d_cap.ptr, d_dig.ptr, True, True)
        assert np.array_equal(d_dig.get()[:4 * num_leaves].reshape(num_leaves, 4), _leaf_hashes(hasher, rows[:, :8]))
    finally:
        for b in (d_cols, d_cap, d_dig):
            b.free()


# ------------------------------------------------------------------------------------------------ proof of work
NONE = M64
WINDOWS = [(0, 1), (0, 5000), ((1 << 32) - 100, 300), ((1 << 40) + 3, 4097), (1 << 63, 257)]
SEEDS = [[0, M64, 0x0123456789ABCDEF, P, 1 << 63], [0xD1B54A32D192ED03, 0x9E3779B97F4A7C15, 0xFFFFFFFF00000000, 7, P - 1]]
POW_BITS = [0, 1, 4, 12, 40]


def _seed_bytes(seed):
    return np.array(seed, dtype="<u8").tobytes()


@functools.lru_cache(maxsize=None)
def _trailing_zeros(runner, seed_id, base, count):
    """Trailing zeros of the reference's first digest word for every nonce of the window (64 for the word 0)."""
    words = OP._pow_first_words(_seed_bytes(SEEDS[seed_id]), [base + i for i in range(count)], runner)
    return [64 if w == 0 else (w & -w).bit_length() - 1 for w in words]


def _smallest(tz, base, bits, start=0):
    return next((base + i for i in range(start, len(tz)) if tz[i] >= bits), NONE)


both_runners = pytest.mark.parametrize("runner", [POW_BLAKE2S256, POW_KECCAK256], ids=["blake2s", "keccak"])


@both_runners
@pytest.mark.parametrize("base,count", WINDOWS)
def test_pow_search_is_the_smallest_accepted_nonce(runner, base, count):
    """Every window at pow_bits 0 (the answer is base), 1 and 4 (many hits: the minimum), 12 and 40 (most likely none: ~0), for
    two seeds; expected is whatever the reference gives for the window."""
    for seed_id, seed in enumerate(SEEDS):
        tz = _trailing_zeros(runner, seed_id, base, count)
        for bits in POW_BITS:
            want = _smallest(tz, base, bits)
            if bits == 0:
                assert want == base
            assert ctx().pow_search(runner, seed, bits, base, count) == want, (seed_id, bits)
        assert ctx().pow_search(runner, seed, 64, base, count) == _smallest(tz, base, 64)


@both_runners
@pytest.mark.parametrize("base,count", WINDOWS[1:])
def test_pow_search_minimum_and_window_end(runner, base, count):
    """Of several hits the smallest: after the reference's first hit at 4 bits the search over [hit + 1, ...) gives the next one.
    And a window that ends right before a hit does not return it."""
    seed = SEEDS[1]
    tz = _trailing_zeros(runner, 1, base, count)
    hits = [i for i in range(count) if tz[i] >= 4]
    assert len(hits) >= 3                                   # 300 nonces at 2^-4 each: fewer than three hits has probability 2e-6
    for k in range(2):
        start = hits[k] + 1
        assert ctx().pow_search(runner, seed, 4, base + start, count - start) == base + hits[k + 1]
    lo = hits[0] + 1                                        # (hit 0, hit 1): no hit inside, one right behind
    if hits[1] > lo:
        assert ctx().pow_search(runner, seed, 4, base + lo, hits[1] - lo) == NONE
    assert ctx().pow_search(runner, seed, 4, base + lo, hits[1] - lo + 1) == base + hits[1]


@both_runners
def test_pow_search_is_the_provers_search(runner):
    """oracle.prover.pow_search at 10 bits, the serial search a proof's nonce is checked against, is the door over [0, 2^12)."""
    for seed in SEEDS:
        want = OP.pow_search(_seed_bytes(seed), 10, runner)
        assert want < (1 << 12)                             # these seeds' nonces: 23, 20 (Blake2s), 3236, 135 (Keccak)
        assert ctx().pow_search(runner, seed, 10, 0, 1 << 12) == want


# ------------------------------------------------------------------------------------------------ refusals
def _refused(call, *args, **kw):
    with pytest.raises(E.BoojumHipError):
        call(*args, **kw)


def test_refusals_leave_the_context_usable():
    c = ctx()
    rng = np.random.default_rng(8000)
    n = 256
    mono = rand_gl(rng, (2, n))
    d_mono, d_idx, d_out = DevBuf(mono), DevBuf(np.array([0, 2 * n - 1], dtype=np.uint64)), DevBuf(nelems=4)
    want_eval = horner_rows(mono, 9, [0, 2 * n - 1])

    def eval_ok():
        c.eval_monomials_at(d_mono.ptr, n, 2, 8, 1, d_idx.ptr, 2, d_out.ptr)
        assert np.array_equal(d_out.get((2, 2)), want_eval)

    try:
        eval_ok()
        for bad in (dict(d_mono=None), dict(d_idx=None), dict(d_out=None), dict(col_stride=n - 1), dict(tiled=True),
                    dict(log_n=21, tiled=True), dict(first_leaf=2 * n), dict(log_lde=30)):
            a = dict(d_mono=d_mono.ptr, col_stride=n, n_cols=2, log_n=8, log_lde=1, d_idx=d_idx.ptr, n_idx=2, d_out=d_out.ptr)
            a.update(bad)
            _refused(c.eval_monomials_at, **a)
            eval_ok()
    finally:
        for b in (d_mono, d_idx, d_out):
            b.free()

    leaves = 100
    cols = rand_gl(rng, (8, leaves))
    d_cols, d_cap, d_dig = DevBuf(cols), DevBuf(nelems=4 * leaves), DevBuf(nelems=4 * leaves)
    want_dig = np.stack([O.hash_leaf(r) for r in cols.T])

    def absorb_ok():
        c.set_tree_hasher(HASHER_POSEIDON2)
        c.merkle_leaves_absorb(d_cols.ptr, leaves, 8, leaves, d_cap.ptr, d_dig.ptr, True, True)
        assert np.array_equal(d_dig.get((leaves, 4)), want_dig)

    try:
        absorb_ok()
        for byte_hasher in (HASHER_BLAKE2S, HASHER_KECCAK256):
            c.set_tree_hasher(byte_hasher)
            _refused(c.merkle_leaves_absorb, d_cols.ptr, leaves, 8, leaves, d_cap.ptr, d_dig.ptr, True, True)
            absorb_ok()
        for args in ((d_cols.ptr, leaves, 0, leaves, d_cap.ptr, d_dig.ptr, True, True),         # no columns
                     (d_cols.ptr, leaves, 7, leaves, d_cap.ptr, d_dig.ptr, True, False),        # 7 columns, not the last group
                     (d_cols.ptr, leaves, 12, leaves, d_cap.ptr, d_dig.ptr, False, False),
                     (d_cols.ptr, leaves - 1, 8, leaves, d_cap.ptr, d_dig.ptr, True, True),     # stride below the leaf count
                     (None, leaves, 8, leaves, d_cap.ptr, d_dig.ptr, True, True),
                     (d_cols.ptr, leaves, 8, leaves, None, d_dig.ptr, False, True),
                     (d_cols.ptr, leaves, 8, leaves, d_cap.ptr, None, True, True),
                     (d_cols.ptr, leaves, 8, 0, d_cap.ptr, d_dig.ptr, True, True)):
            _refused(c.merkle_leaves_absorb, *args)
            absorb_ok()
    finally:
        c.set_tree_hasher(HASHER_POSEIDON2)
        for b in (d_cols, d_cap, d_dig):
            b.free()

    seed = SEEDS[1]
    want_pow = _smallest(_trailing_zeros(POW_BLAKE2S256, 1, 0, 5000), 0, 4)

    def pow_ok():
        assert c.pow_search(POW_BLAKE2S256, seed, 4, 0, 5000) == want_pow

    pow_ok()
    for args in ((0, seed, 4, 0, 16), (3, seed, 4, 0, 16), (-1, seed, 4, 0, 16),                # runner
                 (POW_BLAKE2S256, seed, 4, 0, 0), (POW_KECCAK256, seed, 4, 0, (1 << 24) + 1),    # count
                 (POW_BLAKE2S256, seed, 65, 0, 16),                                               # pow_bits
                 (POW_BLAKE2S256, seed, 4, M64 - 15, 16), (POW_KECCAK256, seed, 4, M64, 1), (POW_BLAKE2S256, seed, 4, M64 - 3, 1 << 24)):
        _refused(c.pow_search, *args)
        pow_ok()
    assert c.pow_search(POW_BLAKE2S256, seed, 0, M64 - 16, 16) == M64 - 16                       # the last window that is taken
