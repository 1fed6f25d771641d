"""The constructions of tests/poseidon2_tree_cases.py on the CPU: the integer sponge against the oracle, and every constructed
case against the claim it carries (which S-box words of which block see the target, which class the named product takes, which
output word of the first external layer wraps under the model of its kernel).  The GPU side, which runs these cases through the
five Poseidon2 tree kernels, is tests/test_gpu_poseidon2_tree_kernels.py; no parametrisation of it can pass on an empty list."""
import numpy as np
import pytest

import oracle as O

import poseidon2_tree_cases as TC
import poseidon_rare as PR

P = PR.P


def _noncanonical(rng, shape):
    a = rng.integers(0, P, size=shape, dtype=np.uint64)
    pick = rng.random(size=shape) < 0.25
    return np.where(pick, np.uint64(P) + rng.integers(0, (1 << 32) - 1, size=shape, dtype=np.uint64), a)


def test_integer_permutation_equals_the_oracle():
    rng = np.random.default_rng(5)
    states = list(_noncanonical(rng, (12, 12))) + [np.zeros(12, dtype=np.uint64), np.full(12, (1 << 64) - 1, dtype=np.uint64)]
    for st in states:
        out, first = TC.permutation([int(x) for x in st])
        assert out == [int(x) for x in O.poseidon2_permutation(st)]
        assert first == [(x + r) % P for x, r in zip(PR.p2_ext_mds([int(v) % P for v in st]), PR.RC[0])]


@pytest.mark.parametrize("width", [1, 7, 8, 9, 16, 17, 128])
def test_integer_sponge_equals_hash_leaf(width):
    rng = np.random.default_rng(20 + width)
    for leaf in _noncanonical(rng, (6, width)):
        log, digest = TC.sponge(TC.rate_blocks(leaf))
        assert len(log) == (width + 7) // 8
        assert digest == [int(x) for x in O.hash_leaf(leaf)]


@pytest.mark.parametrize("elems", [1, 2, 4, 8, 64])
def test_integer_sponge_equals_the_chunked_tree(elems):
    rng = np.random.default_rng(40 + elems)
    leaves, cap = 8, 2
    src = _noncanonical(rng, (2, leaves * elems))
    tree = O.merkle_construct_chunked(src, elems, cap)
    digests = []
    for j in range(leaves):
        words = list(src[0, j * elems:(j + 1) * elems]) + list(src[1, j * elems:(j + 1) * elems])
        digests.append(TC.sponge(TC.rate_blocks(words))[1])
        assert digests[j] == [int(x) for x in tree[j]], j
    for i in range(leaves // 2):                                # a parent is the sponge over its two children
        assert TC.sponge([digests[2 * i] + digests[2 * i + 1]])[1] == [int(x) for x in tree[leaves + i]], i


@pytest.mark.parametrize("cls", [1, 3])
@pytest.mark.parametrize("second_block", [False, True])
def test_sbox_cases_show_their_target(cls, second_block):
    cases = TC.sbox_cases(cls, np.random.default_rng(60 + cls), second_block)
    assert cases
    words_seen = set()
    for c in cases:
        assert len(c["words"]) == (16 if second_block else 8) and all(0 <= w < P for w in c["words"])
        log, _ = TC.sponge(TC.rate_blocks(c["words"]))
        assert c["block"] == int(second_block) and c["rows"]
        assert all(log[c["block"]][k] == c["x"] for k in c["rows"]), c
        assert c["x"] >= (1 << 32) - 1
        a, b = PR.pow7_operands(c["x"], "weak")[PR.PRODUCTS.index(c["product"])]
        assert PR.mul_weak_model(a, b)[1] == cls, c
        words_seen.update(c["rows"])
    assert words_seen == set(range(12))
    assert any(len(c["rows"]) == 8 for c in cases) and {c["rows"] for c in cases if len(c["rows"]) == 1} >= {(0,), (5,), (8,), (11,)}


def test_sbox_targets_of_both_classes():
    t1, t3 = TC.sbox_targets(1), TC.sbox_targets(3)
    assert {x for x, _ in t1} >= {1 << 48, 3 << 48} and all(prod == "x*x" for _, prod in t1)
    assert {prod for _, prod in t3} == set(PR.PRODUCTS)        # class 3 is driven at every product of x^7
    assert {x for x, _ in t1 + t3} >= {e["x"] for e in PR.entries("weak", 1) + PR.entries("weak", 3)}


def test_eight_free_words_reach_only_these_row_sets():
    """The count behind ROW_SETS: most eight-row systems over the eight rate words are singular mod p."""
    from itertools import combinations
    singular = 0
    for rows in combinations(range(12), 8):
        try:
            PR.solve_mod_p(TC._sub(rows), [0] * 8)
        except StopIteration:                                   # no pivot
            singular += 1
    assert singular == 414


@pytest.mark.parametrize("model", ["stream", "stream_folded", "lanepar"])
def test_carry_cases_wrap_at_their_word(model):
    cases = TC.carry_cases(model, np.random.default_rng(80))   # asserts each case and the union itself
    assert len(cases) == 48 and {c["word"] for c in cases} == set(range(12))
    reached = set()
    for c in cases:
        st = c["words"] + [0] * 4
        assert all(w < P for w in c["words"])
        hit = TC.CARRY_MODELS[model](st, PR.RC[0])
        assert c["word"] in hit
        reached.update(hit)
    assert reached == set(range(12))
    for lows in ("ones", "random"):                             # the GPU tests take one kind of low halves per case list
        assert {c["word"] for c in TC.carry_cases(model, np.random.default_rng(82), reps=1, low_halves=(lows,))} == set(range(12))


@pytest.mark.parametrize("model", ["stream", "stream_folded", "lanepar"])
def test_plane_sums_recombine_to_the_layer(model):
    """Each model's planes are the first external layer: A + 2^32 * B is EXT * state, plus RC[0] where the kernel's planes carry
    the constant (the lane-parallel kernel adds it after the fold)."""
    rng = np.random.default_rng(83)
    k_lo, k_hi = TC.CARRY_CONSTANTS[model](PR.RC[0])
    for _ in range(8):
        st = [int(x) for x in rng.integers(0, 1 << 63, size=8, dtype=np.uint64) * 2 + 1] + [0] * 4
        want = [(x + (0 if model == "lanepar" else r)) % P for x, r in zip(PR.p2_ext_mds([x % P for x in st]), PR.RC[0])]
        sums = TC.plane_sums(st, k_lo, k_hi)
        assert [(A + (B << 32)) % P for A, B in sums] == want
        assert all(A < 1 << 48 and B < 1 << 48 for A, B in sums)              # the bound the stream's fold assumes


def test_the_carry_models_differ():
    """The constants move the wrap: cases built for one model are not all cases of another, so each kernel gets the cases of the
    model of its own planes."""
    for built, other in (("lanepar", "stream"), ("stream_folded", "stream"), ("stream_folded", "lanepar")):
        cases = TC.carry_cases(built, np.random.default_rng(81))
        assert any(c["word"] not in TC.CARRY_MODELS[other](c["words"] + [0] * 4, PR.RC[0]) for c in cases), (built, other)
    st = TC.carry_cases("lanepar", np.random.default_rng(81))[0]["words"] + [0] * 4     # the lane-parallel model restated
    for i in range(12):
        A = sum(PR.EXT[i][j] * (st[j] & 0xFFFFFFFF) for j in range(12))
        B = sum(PR.EXT[i][j] * (st[j] >> 32) for j in range(12))
        T = A + (B >> 32) * ((1 << 32) - 1)
        assert ((T >> 32) + (B & 0xFFFFFFFF) >= 1 << 32) == (i in TC.lanepar_carry_words(st))


def test_spread16_layout():
    cases = np.arange(3 * 8, dtype=np.uint64).reshape(3, 8) + np.uint64(1)
    rows, lone, whole = TC.spread16(cases, lambda n: np.zeros((n, 8), dtype=np.uint64))
    assert rows.shape == (2 * 3 * 16, 8)
    for c in range(3):
        assert lone[c] // 16 == c and np.array_equal(rows[lone[c]], cases[c])
        assert sum(bool(r.any()) for r in rows[16 * c:16 * c + 16]) == 1           # alone in its slice
        assert whole[c] % 16 == 0 and all(np.array_equal(r, cases[c]) for r in rows[whole[c]:whole[c] + 16])
