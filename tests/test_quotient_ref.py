"""tests/quotient_ref.py (the quotient-term operators restated from their definitions in python integers) against the oracle on a
satisfied circuit: the three terms applied in the prover's order equal OP.quotient word for word, each term alone does, and
lookup_polys_ref equals OP.lookup_polys.  tests/test_gpu_quotient_terms.py then holds the device to the same functions on
columns no circuit produces.  No GPU."""
import numpy as np
import pytest

import quotient_cases as QC
import quotient_ref as R
from era_boojum_amd import field_np
from oracle import prover as OP
from quotient_cases import BETA, GAMMA, LBETA, LGAMMA

_shared = {}


def _inputs(kw):
    key = tuple(sorted(kw.items()))
    if key not in _shared:
        c = QC.circuit(9, **kw)
        _shared[key] = (c, QC.quotient_inputs(c))
    return _shared[key]


def _reference_terms(c, d, alphas):
    """gates (overwrites), lookup (adds), copy permutation (adds, then divides by x^n - 1): the prover's order"""
    Q, nl, ng, n_part, reps = d["Q"], d["n_lookup"], d["n_gate"], d["n_part"], c.lookup_reps
    a_lookup, a_gates, a_cp = alphas[:nl], alphas[nl:nl + ng], alphas[nl + ng:]
    T = R.gates_term(d["vars"][:c.num_gp_vars], d["con"], c.gates, a_gates, Q)
    lv = d["vars"][c.num_gp_vars:]
    tid = None if c.table_id_as_variable else d["con"][c.table_id_col]
    A, B = d["s2"][2 + 2 * n_part:2 + 2 * n_part + 2 * reps], d["s2"][2 + 2 * n_part + 2 * reps:]
    T = R.lookup_term(lv, tid, d["tab"], d["mult"], A, B, reps, c.lookup_width, LBETA, LGAMMA, a_lookup, Q, T)
    T = R.copy_perm_term(d["vars"], d["sig"], d["s2"][:2 + 2 * n_part], c.non_residues, c.quotient_degree, c.log_n, d["log_q"],
                         BETA, GAMMA, a_cp, 0, Q, T)
    return R.to_words(*T)


def test_domain_constants():
    assert R.P == QC.P == field_np.P
    assert R.ROOT_2_32 == 0x185629DCDA58878C and pow(R.ROOT_2_32, 1 << 31, R.P) == R.P - 1
    for log_size in (1, 6, 11):
        assert R.omega(log_size) == field_np.omega(log_size)
    # x^n is constant on a coset and is what coset_xn says
    log_n, log_lde = 4, 3
    x = R.lde_points(log_n, log_lde, 0, 16 << log_lde)
    for I, xi in enumerate(x):
        assert pow(int(xi), 16, R.P) == R.coset_xn(log_n, log_lde, I >> log_n)
        assert x[R.next_in_coset(I, log_n)] == xi * R.omega(log_n) % R.P


@pytest.mark.parametrize("kw", [{}, dict(table_id_as_variable=True)], ids=["table_id_constant", "table_id_variable"])
def test_reference_terms_equal_the_oracle_quotient(kw):
    c, d = _inputs(kw)
    al, nl, ng, nch = d["alphas"], d["n_lookup"], d["n_gate"], d["n_chunks"]
    zero = [(0, 0)]
    assert np.array_equal(_reference_terms(c, d, al), QC.oracle_quotient(c, d, al))
    # each term alone (the others' challenges zero): a slip in one term cannot hide behind another
    for alphas in (zero * nl + al[nl:nl + ng] + zero * (1 + nch), al[:nl] + zero * (ng + 1 + nch), zero * (nl + ng) + al[nl + ng:]):
        want = QC.oracle_quotient(c, d, alphas)
        assert want.any()
        assert np.array_equal(_reference_terms(c, d, alphas), want)


def test_reference_terms_equal_the_oracle_quotient_when_z_is_not_one():
    """The circuit's copy constraints join cells of one row, so its z is 1 everywhere: (z - 1) L1 vanishes and z(omega x) = z(x).
    The oracle's quotient is the same pointwise function of whatever columns it is given: with random words for the two z
    columns the L1 term and the shifted z are pinned as well (all terms, the copy-permutation terms alone, the L1 term alone)."""
    c, d = _inputs({})
    assert (d["s2"][0] == 1).all() and not d["s2"][1].any()
    d = dict(d)
    d["s2"] = d["s2"].copy()
    d["s2"][0:2] = np.random.default_rng(5).integers(0, R.P, size=(2, d["Q"]), dtype=np.uint64)
    al, nl, ng, nch = d["alphas"], d["n_lookup"], d["n_gate"], d["n_chunks"]
    zero = [(0, 0)]
    for alphas in (al, zero * (nl + ng) + al[nl + ng:], zero * (nl + ng) + al[nl + ng:nl + ng + 1] + zero * nch):
        want = QC.oracle_quotient(c, d, alphas)
        assert want.any()
        assert np.array_equal(_reference_terms(c, d, alphas), want)


def test_reference_gate_term_with_another_gate_list_equals_the_oracle():
    """The circuit's own gates come in one order with paths of two constants and a constant stride of 1.  Over the same LDE
    columns (the oracle evaluates whatever gate list it is given): another order, paths of 0, 1 and 3 constants, allocations
    that take every other constant column, and a gate that spends no power between them."""
    import copy
    from era_boojum_amd.synthetic import GATE_CONSTANT_ALLOCATOR, GATE_FMA, GATE_NOP, GATE_REDUCTION4, GateDesc
    c, d = _inputs({})
    assert d["con"].shape[0] >= 6
    c2, d2 = copy.copy(c), dict(d)
    c2.gates = [GateDesc(GATE_REDUCTION4, "ReductionGate<4>", 2, 4, 5, 3, 5, 0, 1, True, path=[True]),
                GateDesc(GATE_NOP, "NopGate", 0, 0, 0, 1, 0, 0, 0, True),
                GateDesc(GATE_CONSTANT_ALLOCATOR, "ConstantsAllocatorGate", 1, 1, 1, 2, 1, 2, 1, True, path=[False, True, True]),
                GateDesc(GATE_FMA, "FmaGateInBaseFieldWithoutConstant", 3, 2, 4, 4, 4, 0, 1, True, path=[])]
    d2["n_gate"] = ng = 9
    nl, nch = d["n_lookup"], d["n_chunks"]
    alphas = [(0, 0)] * nl + d["alphas"][5:5 + ng] + [(0, 0)] * (1 + nch)
    want = QC.oracle_quotient(c2, d2, alphas)
    assert want.any()
    assert np.array_equal(_reference_terms(c2, d2, alphas), want)


def test_reference_copy_permutation_term_on_a_coset_range():
    """The points of one coset alone equal the same slice of the whole domain's term."""
    c, d = _inputs({})
    n, Q, n_part = c.n, d["Q"], d["n_part"]
    a_cp = d["alphas"][d["n_lookup"] + d["n_gate"]:]
    zeros = lambda m: (np.zeros(m, dtype=object), np.zeros(m, dtype=object))
    args = (d["vars"], d["sig"], d["s2"][:2 + 2 * n_part], c.non_residues, c.quotient_degree, c.log_n, d["log_q"], BETA, GAMMA, a_cp)
    whole = R.to_words(*R.copy_perm_term(*args, 0, Q, zeros(Q)))
    for first, count in ((2 * n, n), (3 * n, n // 2)):
        part = R.to_words(*R.copy_perm_term(*args, first, count, zeros(count)))
        assert np.array_equal(part, whole[:, first:first + count])


@pytest.mark.parametrize("kw", [{}, dict(table_id_as_variable=True)], ids=["table_id_constant", "table_id_variable"])
def test_reference_lookup_polynomials_equal_the_oracle(kw):
    c, _ = _inputs(kw)
    lv, tid = QC.lookup_vars(c), OP.lookup_table_id(c, c.constants)
    wA, wB = OP.lookup_polys(lv, tid, c.tables, c.multiplicities[0], c.lookup_reps, c.lookup_width, c.log_n, LBETA, LGAMMA, threads=4)
    A, B = R.lookup_polys_ref(lv, tid, c.tables, c.multiplicities[0], c.lookup_reps, c.lookup_width, c.n, LBETA, LGAMMA)
    assert np.array_equal(A, wA) and np.array_equal(B, wB)


def test_reference_gate_program_semantics_equal_the_programs_own():
    """The op-list gate the device test places between the hand-written ones: this module's reading of an op list against
    GateProgram.evaluate, term by term."""
    from era_boojum_amd import gate_program as GP
    rng = np.random.default_rng(11)
    for prog, width, n_const in ((GP.selection_program(), 4, 0), (GP.uintx_add_program(), 5, 1), (GP.zero_check_program(), 3, 0)):
        var, con = QC.raw_columns(rng, width, 40, 40), QC.raw_columns(rng, max(1, n_const), 40, 40)
        got = R._run_program(prog, lambda k: R.res(var[k]), lambda k: R.res(con[k]))
        for i in range(40):
            want = prog.evaluate([int(x) for x in var[:, i]], [int(x) for x in con[:, i]])
            assert [int(np.broadcast_to(t, (40,))[i]) % R.P for t in got] == want


def test_lookup_polys_cases_of_the_device_test_have_no_zero_denominator():
    for w, reps, tid_var, nc in QC.lookup_polys_cases():
        k = QC.lookup_polys_case(w, reps, tid_var, nc)
        for d in R.lookup_denominators(k["lvars"], k["tid"], k["tables"], reps, w, k["lbeta"], k["lgamma"], k["n"]):
            assert not ((d[0] == 0) & (d[1] == 0)).any(), (w, reps, tid_var, nc)


def test_raw_columns_plant_every_edge_word():
    rng = np.random.default_rng(1)
    a = QC.raw_columns(rng, 3, 700, 650, salt=2)
    for k, word in enumerate(QC.EDGE_WORDS):
        assert (a[:, 5 + 7 * ((k - 2) % 9)] == np.uint64(word)).all()                      # the lone lane, a whole row
        for c in range(3):
            assert any((a[c, 64 * (j + 1):64 * (j + 2)] == np.uint64(word)).all() for j in range(9))   # a whole wave, every column
    share = (a[:, 650:] >= np.uint64(QC.P)).mean()
    assert 0.1 < share < 0.4
    assert [int(x) for x in QC.raw_columns(rng, 3, 4, 1)[:, 0]] == QC.EDGE_WORDS[:3]
