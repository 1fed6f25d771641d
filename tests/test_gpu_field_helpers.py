"""-m gpu parity of the csrc/gl.h helpers that run on the device through other code than on the host, or that only whole kernels
on random columns reach: operators 12-23 of bj_field_op_batch against Python integers, every word equal and canonical.

gl::reduce_limbs and gl::mul_limbs are inline assembly on the device (multiply-adds whose carry masks are read a hand-counted
number of wait states later); they run only under gl::Acc160 — the lazy accumulator of every quotient-term kernel, the openings,
the verifier and the gate evaluators — and in check_satisfied.hip.  Random data takes the borrow and the "no carry but r >= p"
branches of the reduction once in 2^32, so the vectors of tests/field_helper_cases.py put every branch class on a lone lane, on
whole waves, on a wave and one lane, and next to every other class inside one wave.  tests/test_field_helper_cases.py proves
on the CPU which branch each vector takes."""
from unittest import mock

import numpy as np
import pytest

import era_boojum_amd as E
import field_helper_cases as C
from gpu_util import ctx

pytestmark = pytest.mark.gpu
P = C.P
SIZES = (1, 63, 64, 65, 257)


def u64(xs):
    return np.array(xs, dtype=np.uint64)


def same(got, want, inputs, what):
    """Every word equal (the wanted words are canonical, so equality is also canonicity); names the first input that differs."""
    got = [int(x) for x in np.asarray(got).reshape(-1)]
    assert len(got) == len(want), what
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s: %d of %d differ; first at %d: in %s got %#x want %#x" % (
        what, len(bad), len(want), bad[0], [hex(x) for x in inputs[bad[0] % len(inputs)]], got[bad[0]], want[bad[0]])


def cycle(vectors, n, start=0):
    return [vectors[(start + i) % len(vectors)] for i in range(n)]


# ---- 12: gl::reduce128 ------------------------------------------------------------------------------------------------
def run_reduce128(vectors, what):
    got = ctx().field_op("reduce128", u64([(hh << 32) | hl for hh, hl, _ in vectors]), u64([lo for _, _, lo in vectors]))
    same(got, [C.reduce_value(v) % P for v in vectors], vectors, "reduce128 " + what)


@pytest.fixture(scope="module")
def reduce_classes():
    return C.by_class(C.reduction_grid(), lambda v: C.reduce_model(*v)[1])


def test_reduce128_on_the_whole_grid_and_on_random_words():
    rng = np.random.default_rng(12)
    grid = C.reduction_grid()
    run_reduce128(grid, "grid")
    run_reduce128([(int(a) >> 32, int(a) & C.M32, int(b)) for a, b in rng.integers(0, 1 << 64, (1 << 15, 2), dtype=np.uint64)], "random")
    # the form check_satisfied.hip uses: a 32-bit high word
    run_reduce128([(0, hl, lo) for _, hl, lo in grid], "32-bit high word")


@pytest.mark.parametrize("cls", C.CLASSES)
def test_reduce128_each_branch_class_alone(reduce_classes, cls):
    """One class in every lane: a lone lane, a wave less one, a full wave, a wave and one lane, several blocks' worth."""
    vectors = reduce_classes[cls]
    for n in SIZES:
        run_reduce128(cycle(vectors, n, start=n), "%s alone, n = %d" % (cls, n))
    for v in vectors[:8]:
        run_reduce128([v], "%s, one lane" % cls)


def test_reduce128_classes_interleaved_lane_by_lane(reduce_classes):
    mixed = C.interleave(reduce_classes)
    run_reduce128(mixed, "interleaved")
    run_reduce128(mixed[:64], "interleaved, one wave")
    run_reduce128(mixed[5:64], "interleaved, part of a wave")


# ---- 13: gl::Acc160 --------------------------------------------------------------------------------------------------
def run_acc160(vectors, what):
    a = u64([[v[3] for v in vectors], [(v[1] << 32) | v[2] for v in vectors], [v[0] for v in vectors]])
    b = u64([[v[4] for v in vectors], [v[5] for v in vectors]])
    got = ctx().field_op("acc160", a, b)
    assert got.shape == (len(vectors),)
    same(got, [C.acc_sum(v) % P for v in vectors], vectors, "acc160 " + what)


@pytest.fixture(scope="module")
def acc_vectors():
    kept, _ = C.accumulator_grid()
    return kept, C.by_class(kept, lambda v: C.acc160_model(v)[1])


def test_acc160_on_the_whole_grid(acc_vectors):
    kept, _ = acc_vectors
    assert len(kept) <= 1 << 16
    run_acc160(kept, "grid")
    # the top word is the low half of its input word
    rng = np.random.default_rng(13)
    some = kept[::37]
    a = u64([[v[3] for v in some], [(v[1] << 32) | v[2] for v in some], [v[0] | (int(r) << 32) for v, r in zip(some, rng.integers(1, 1 << 32, len(some)))]])
    got = ctx().field_op("acc160", a, u64([[v[4] for v in some], [v[5] for v in some]]))
    same(got, [C.acc_sum(v) % P for v in some], some, "acc160, junk above w4")


@pytest.mark.parametrize("cls", C.CLASSES)
def test_acc160_each_branch_class_alone(acc_vectors, cls):
    """The class is that of the reduction after the product went in."""
    vectors = acc_vectors[1][cls]
    for n in SIZES:
        run_acc160(cycle(vectors, n, start=n), "%s alone, n = %d" % (cls, n))
    with_product = [v for v in vectors if v[4] and v[5]]
    for n in SIZES:
        run_acc160(cycle(with_product, n, start=3 * n), "%s alone, products only, n = %d" % (cls, n))


def test_acc160_classes_interleaved_lane_by_lane(acc_vectors):
    mixed = C.interleave(acc_vectors[1])
    run_acc160(mixed, "interleaved")
    run_acc160(mixed[:64], "interleaved, one wave")
    run_acc160(mixed[5:64], "interleaved, part of a wave")


# ---- 14: gl::Acc160x2::fma_e2 -------------------------------------------------------------------------------------------
def test_acc_ext2_adds_an_extension_product_twice():
    cases = C.acc_ext2_cases()
    for vectors in (cases, cases[:1], cases[:65]):
        a = u64([[v[0] for v in vectors], [v[1] for v in vectors]])
        b = u64([[v[2] for v in vectors], [v[3] for v in vectors]])
        got = ctx().field_op("acc_ext2", a, b)
        want = [C.acc_ext2_want(v) for v in vectors]
        same(got, [w[0] for w in want] + [w[1] for w in want], vectors, "acc_ext2, n = %d" % len(vectors))


# ---- 15-19: small-constant products, x^7 ----------------------------------------------------------------------------------
def test_mul7_lazy():
    a = C.mul7_lazy_cases()
    same(ctx().field_op("mul7_lazy", u64(a)), [7 * x % P for x in a], [(x,) for x in a], "mul7_lazy")


def test_mul_u32_lazy():
    cases = C.mul_u32_cases()
    got = ctx().field_op("mul_u32_lazy", u64([a for a, _ in cases]), u64([k for _, k in cases]))
    same(got, [a * (k & C.M32) % P for a, k in cases], cases, "mul_u32_lazy")
    wrapping = [(a, k) for a, k in cases if C.mul_u32_weak_model(a, k & C.M32)[1]]
    for n in (1, 64, 65):
        v = cycle(wrapping, n)
        got = ctx().field_op("mul_u32_lazy", u64([a for a, _ in v]), u64([k for _, k in v]))
        same(got, [a * (k & C.M32) % P for a, k in v], v, "mul_u32_lazy, wrapping sums alone, n = %d" % n)


def test_mul_pow2():
    cases = C.mul_pow2_cases()
    got = ctx().field_op("mul_pow2", u64([a for a, _ in cases]), u64([k for _, k in cases]))
    same(got, [((a % P) << (k & 31)) % P for a, k in cases], cases, "mul_pow2")


def test_mul7():
    a = C.mul7_cases()
    same(ctx().field_op("mul7", u64(a)), [7 * x % P for x in a], [(x,) for x in a], "mul7")


def test_pow7():
    a = C.pow7_cases()
    same(ctx().field_op("pow7", u64(a)), [pow(x, 7, P) for x in a], [(x,) for x in a], "pow7")


# ---- 20-22: the inversions -------------------------------------------------------------------------------------------------
def test_inverse_chain_equals_square_and_multiply_and_python():
    a = C.inverse_cases()
    want = [pow(x % P, P - 2, P) for x in a]
    same(ctx().field_op("inverse_chain", u64(a)), want, [(x,) for x in a], "inverse_chain")
    same(ctx().field_op("inverse", u64(a)), want, [(x,) for x in a], "inverse")


def test_ext2_inversions_agree_with_each_other_and_with_python():
    cases = C.ext2_inverse_cases()
    a = u64([[v[0] for v in cases], [v[1] for v in cases]])
    want = [C.ext2_inverse_want(v) for v in cases]
    want = [w[0] for w in want] + [w[1] for w in want]
    plain, chain = ctx().field_op("ext2_inverse", a), ctx().field_op("ext2_inverse_chain", a)
    assert plain.shape == a.shape and np.array_equal(plain, chain)
    same(plain, want, cases, "ext2_inverse")
    same(chain, want, cases, "ext2_inverse_chain")


# ---- 23: gl::bitrev32 ----------------------------------------------------------------------------------------------------
def test_bitrev():
    cases = C.bitrev_cases()
    got = ctx().field_op("bitrev", u64([x for x, _ in cases]), u64([b for _, b in cases]))
    same(got, [C.bitrev_want(v) for v in cases], cases, "bitrev")


# ---- the ABI's checks ------------------------------------------------------------------------------------------------
UNARY = ("mul7_lazy", "mul7", "pow7", "inverse_chain", "ext2_inverse", "ext2_inverse_chain")
NEW = ("reduce128", "acc160", "acc_ext2", "mul_u32_lazy", "mul_pow2", "bitrev") + UNARY


def test_new_operators_are_numbered_12_to_23():
    assert sorted(E.Context.FIELD_OPS[op] for op in NEW) == list(range(12, 24))


def test_empty_inputs_succeed():
    empty = np.zeros(0, dtype=np.uint64)
    for op in NEW:
        assert ctx().field_op(op, empty, None if op in UNARY else empty).size == 0


def test_unknown_operator_and_missing_second_operand_are_refused():
    c = ctx()
    one = np.ones(6, dtype=np.uint64)
    with mock.patch.dict(E.Context.FIELD_OPS, {"beyond the last": 24}), pytest.raises(E.BoojumHipError):
        c.field_op("beyond the last", one, one)
    for op in NEW:
        if op not in UNARY:
            with pytest.raises(E.BoojumHipError):
                c.field_op(op, one, None)
    # the context still works after the refusals
    assert int(c.field_op("reduce128", u64([1]), u64([5]))[0]) == ((1 << 64) + 5) % P
