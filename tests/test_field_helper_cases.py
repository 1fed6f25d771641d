"""The vectors of tests/field_helper_cases.py, checked without a GPU: the Python models of the device algorithms equal the
definitions on all of them, every branch class of the device reduction occurs, and a model with one correction taken out fails
on exactly the vectors of that branch — so tests/test_gpu_field_helpers.py cannot pass by an accident of its inputs."""
import field_helper_cases as C

P = C.P


def _cls(v):
    return C.reduce_model(*v)[1]


def test_reduction_grid_reaches_every_branch_class_and_the_model_is_the_definition():
    grid = C.reduction_grid()
    assert len(grid) == len(set(grid)) and all(0 <= hh < 1 << 32 and 0 <= hl < 1 << 32 and 0 <= lo < 1 << 64 for hh, hl, lo in grid)
    classes = C.by_class(grid, _cls)
    print({c: len(v) for c, v in classes.items()}, len(grid))
    assert all(len(classes[c]) >= 16 for c in C.CLASSES), {c: len(v) for c, v in classes.items()}
    assert all(C.reduce_model(*v)[0] == C.reduce_value(v) % P for v in grid)
    # every target of the intermediate sum is met with and without a borrow
    for hh in C.LIMBS[1:]:
        for hl in C.LIMBS:
            los = {lo for a, b, lo in grid if (a, b) == (hh, hl)}
            for target in C.R_TARGETS:
                assert (target - hl * C.EPS + hh) & C.M64 in los


def test_a_reduction_without_one_of_its_corrections_fails_on_exactly_that_branch():
    grid = C.reduction_grid()
    want = [C.reduce_value(v) % P for v in grid]
    no_ge = {v for v, w in zip(grid, want) if C.reduce_model(*v, ge_fix=False)[0] != w}
    assert no_ge == {v for v in grid if _cls(v).endswith("ge")}
    no_borrow = {v for v, w in zip(grid, want) if C.reduce_model(*v, borrow_fix=False)[0] != w}
    assert no_borrow == {v for v in grid if _cls(v).startswith("borrow")}


def test_interleaved_waves_hold_every_class_in_every_wave():
    classes = C.by_class(C.reduction_grid(), _cls)
    mixed = C.interleave(classes)
    assert len(mixed) % 64 == 0
    for w in range(0, len(mixed), 64):
        assert {_cls(v) for v in mixed[w:w + 64]} == set(C.CLASSES)
        assert all(_cls(mixed[w + j]) != _cls(mixed[w + j + 1]) for j in range(63))


def test_accumulator_grid_stays_inside_the_contract_and_reaches_every_class():
    kept, dropped = C.accumulator_grid()
    total = len(kept) + len(dropped)
    print(len(kept), len(dropped), total)
    assert len(dropped) < 0.05 * total
    assert len(kept) <= 1 << 16
    classes = {c: 0 for c in C.CLASSES}
    for v in kept:
        got, cls = C.acc160_model(v)
        assert got == C.acc_sum(v) % P
        classes[cls] += 1
    print(classes)
    assert all(n >= 16 for n in classes.values()), classes
    # the parts the grid is made of are all there
    assert {v[0] for v in kept} >= set(C.W4S)
    assert any(v[4:] == (0, 0) for v in kept) and any(v[4:] == (C.M64, C.M64) for v in kept)
    assert set(C.rare_pairs()) <= {v[4:] for v in kept}
    # one product carries through four all-ones words into the top word
    assert any(v[:4] == (0, C.M32, C.M32, C.M64) and C.acc_sum(v) >> 128 == 1 for v in kept)
    # 2^32 - 1 all-ones products and one more fill the top word: 2^32 (2^64 - 1)^2 = 2^160 - 2^97 + 2^32
    last = C.closed_form_all_ones((1 << 32) - 1) + (C.M64, C.M64)
    assert last in kept and C.acc_sum(last) == (1 << 160) - (1 << 97) + (1 << 32)
    assert all(C.acc_sum(v) >= 1 << 160 for v in dropped)


def test_weak_small_products_wrap_and_do_not_wrap():
    for cases in (C.mul_u32_cases(), [(a, 7) for a in C.mul7_lazy_cases()]):
        outcomes = {False: 0, True: 0}
        for a, k in cases:
            got, wrapped = C.mul_u32_weak_model(a, k & C.M32)
            assert got <= C.M64 and got % P == a * (k & C.M32) % P
            outcomes[wrapped] += 1
        print(outcomes)
        assert outcomes[False] >= 16 and outcomes[True] >= 16
    ks = {k for _, k in C.mul_u32_cases()}
    assert ks >= set(C.KS) and len(ks) > 1000


def test_the_other_vectors_cover_what_they_claim():
    assert {k & 31 for _, k in C.mul_pow2_cases()} == set(range(32))
    assert {P // 7 - 1, P // 7, P // 7 + 1, 0, 1, P - 1} <= set(C.mul7_cases())
    assert any(x >= P for x in C.pow7_cases())
    assert {(a, b) for a in C.INV_SPECIALS for b in C.INV_SPECIALS} <= set(C.ext2_inverse_cases())
    assert len(C.inverse_cases()) >= 2048 and len(C.ext2_inverse_cases()) >= 2048
    for v in C.ext2_inverse_cases():
        c0, c1 = v[0] % P, v[1] % P
        i0, i1 = C.ext2_inverse_want(v)
        if (c0, c1) == (0, 0):
            assert (i0, i1) == (0, 0)
        else:
            assert ((c0 * i0 + 7 * c1 * i1) % P, (c0 * i1 + c1 * i0) % P) == (1, 0)
    assert {bits for _, bits in C.bitrev_cases()} == set(range(33))
    assert C.bitrev_want((0b1011, 4)) == 0b1101 and C.bitrev_want((1, 32)) == 1 << 31 and C.bitrev_want((C.M32, 0)) == 0
    assert all(C.bitrev_want((x & C.M32, 32)) == int("{:032b}".format(x & C.M32)[::-1], 2) for x, _ in C.bitrev_cases())
