"""-m gpu: operator 32 of bj_field_op_batch — gl::w16_butterfly2_weak, the generated gfx950 sequences for the butterflies by 16th
roots of unity (shifts, no product), two per thread as the radix-16 NTT steps run them — on the vectors of tests/w16_cases.py, word
for word against Python integers mod p after canon (tests/test_w16_shift_host.py checks the host side of the same helpers on the
same vectors).  The sequences hand a borrow of the 2^36 / 2^48 / 2^60 products and second wraps of the sum or the difference to a
wave-uniform canonical path: the vectors hold words that take it (the 'borrow' words of those shifts, u = 2^64 - 1 against wrapping
products) next to words that do not, and a launch of random pairs alone, where a wave takes it about once in 2^25 butterflies."""
import numpy as np
import pytest

import w16_cases as C
from gpu_util import ctx

pytestmark = pytest.mark.gpu


def _run(pairs, sel):
    """pairs through selector sel: the first half of the threads' pairs take exponent PAIRS[sel][0], the second half [1]"""
    u = np.array([p[0] for p in pairs], dtype=np.uint64)
    v = np.array([p[1] for p in pairs], dtype=np.uint64)
    a = np.stack([np.concatenate([u, u]), np.concatenate([v, v])])        # both halves see every pair
    b = np.full(a.shape[1], sel, dtype=np.uint64)
    return ctx().field_op("w16_butterfly", a, b)


@pytest.fixture(scope="module")
def vectors():
    return C.pairs(2000)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("sel", range(12))
def test_device_butterflies_equal_python_integers(vectors, sel, inverse):
    ea, eb = C.PAIRS[sel]
    got = _run(vectors, sel | (16 if inverse else 0))
    n = len(vectors)
    want = np.empty((2, 2 * n), dtype=np.uint64)
    for i, (u, v) in enumerate(vectors):
        want[0, i], want[1, i] = C.butterfly(u, v, ea, inverse)
        want[0, n + i], want[1, n + i] = C.butterfly(u, v, eb, inverse)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(r), int(i), hex(vectors[i % n][0]), hex(vectors[i % n][1])) for r, i in bad[:5]]


def test_random_waves_take_the_fast_path_and_agree():
    """64 K random pairs alone: no lane of these waves is a constructed slow-path word"""
    rng = np.random.default_rng(16)
    u = rng.integers(0, 2**64, size=1 << 16, dtype=np.uint64)
    v = rng.integers(0, 2**64, size=1 << 16, dtype=np.uint64)
    for sel in (9, 16 | 11):
        ea, eb = C.PAIRS[sel & 15]
        got = ctx().field_op("w16_butterfly", np.stack([u, v]), np.full(u.size, sel, dtype=np.uint64))
        h = u.size // 2
        for lo, hi, e in ((0, h, ea), (h, 2 * h, eb)):
            w = C.root(e, bool(sel & 16))
            t = [int(x) * w % C.P for x in v[lo:hi]]
            assert [int(x) for x in got[0, lo:hi]] == [(int(x) + y) % C.P for x, y in zip(u[lo:hi], t)]
            assert [int(x) for x in got[1, lo:hi]] == [(int(x) - y) % C.P for x, y in zip(u[lo:hi], t)]
