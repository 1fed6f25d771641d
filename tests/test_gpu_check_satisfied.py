"""-m gpu: bj_check_satisfied (csrc/check_satisfied.hip) against the exact restatement tests/satisfiability_ref.py, field by
field: satisfied circuits of every evaluator kind, one planted failure per kind, lookups and multiplicities in both table-id
modes, non-canonical cells, the from-dumps form, neutrality towards proofs (single and sharded), agreement with the prover."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding
from gpu_util import ctx

import satisfiability_cases as K
import satisfiability_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def setup(name, relooked=0):
    c = K.relooked(name, relooked) if relooked else K.circuit(name)
    return E.ProverSetup(ctx(), c, 8, 16, 30)


def agree(s, full=None, multiplicities=None, want=None):
    """The GPU report equals the restatement's (or `want`), every field."""
    c = s.circuit
    want = R.check(c, full, multiplicities) if want is None else want
    got = s.check_satisfied(K.full_witness(c) if full is None else full, multiplicities)
    assert (got.kind, got.gate, got.repetition, got.term, got.row, got.value, got.expected, got.failures) == want.fields()
    assert bool(got) == (want.kind == R.SAT)
    return got


@pytest.mark.parametrize("name", K.SATISFIED + ["seams10", "extended10", "spec10"])
def test_satisfied_circuits(name):
    got = agree(setup(name))
    assert got.kind == binding.SAT and got.failures == (0, 0, 0, 0, 0) and str(got) == "Satisfied"


# one per evaluator kind: constant allocator, FMA (both sides of the reduction's block seam), Reduction4 on the last row,
# generated op list, run-time compiled op list, both Poseidon gates, a gate that reads a witness column
GATE_CASES = [("seams10", "ConstantsAllocatorGate", 0), ("seams10", "FmaGateInBaseFieldWithoutConstant", 255),
              ("seams10", "FmaGateInBaseFieldWithoutConstant", 256), ("seams10", "ReductionGate<4>", 1023),
              ("extended10", "UIntXAddGate", None), ("jit10", "MatrixMultiplicationGate[host]", None),
              ("golden10", "Poseidon2FlattenedGate", None), ("poseidon1", "PoseidonFlattenedGate", None),
              ("witness10", "ZeroCheckGate[witness]", None), ("sha16", "ReductionGate<4>", (1 << 16) - 1)]


@pytest.mark.parametrize("name,gate,row", GATE_CASES)
def test_planted_gate_failure(name, gate, row):
    s = setup(name)
    c = s.circuit
    gi = K.gate_index(c, gate)
    row = int(K.gate_rows(c, gi)[-1]) if row is None else row
    full, (g, r, t) = K.plant_gate(c, gi, row)
    got = agree(s, full)
    assert (got.kind, got.gate, got.repetition, got.term, got.row) == (binding.UNSAT_GATE, g, r, t, row) and got.failures[1] == 1
    assert str(got) == "Unsatisfied at row %d with value %d for term number %d for subinstance number %d of gate %s" % (row, got.value, t, r, gate)
    # the prover agrees: it refuses this witness and proves the untouched one
    d_v, d_m = ctx().upload(full), ctx().upload(c.multiplicities)
    try:
        with pytest.raises(E.BoojumHipError, match="not satisfied"):
            s.prove_dev(d_v, d_m)
    finally:
        ctx().free(d_v)
        ctx().free(d_m)
    if name != "sha16":
        s.prove()


def test_two_failures_and_both_gate_kinds():
    s = setup("seams10")
    fma = K.gate_index(s.circuit, "FmaGateInBaseFieldWithoutConstant")
    full, _ = K.plant_gate(s.circuit, fma, 300)
    full, _ = K.plant_gate(s.circuit, fma, 256, full)
    got = agree(s, full)
    assert (got.row, got.failures[1]) == (256, 2)
    s = setup("spec10")
    c = s.circuit
    for si, row in ((0, 0), (1, c.n - 1)):
        full, where = K.plant_specialized(c, si, row)
        got = agree(s, full)
        assert (got.kind, got.row, (got.gate, got.repetition, got.term)) == (binding.UNSAT_SPECIALIZED_GATE, row, where)
    red = K.gate_index(c, "ReductionGate<4>")
    full, _ = K.plant_gate(c, red, int(K.gate_rows(c, red)[0]), full)
    got = agree(s, full)
    assert got.kind == binding.UNSAT_GATE and got.failures == (0, 1, 1, 0, 0)


@pytest.mark.parametrize("name,relooked", [("sha10", 0), ("tidvar13", 0), ("sha10", 16), ("sha10", 1021), ("tidvar13", 16)])
def test_lookups_and_multiplicities(name, relooked):
    s = setup(name, relooked)
    c = s.circuit
    n, last = c.n, c.lookup_reps - 1
    agree(s)
    for row, sub in ((0, 0), (n - 1, last)):
        got = agree(s, K.plant_lookup_miss(c, row, sub))
        assert (got.kind, got.row, got.gate, got.failures[3]) == (binding.UNSAT_LOOKUP, row, sub, 1)
    full, (old, new) = K.plant_lookup_swap(c, 77, 3)
    got = agree(s, full)
    assert (got.kind, got.failures[4]) == (binding.UNSAT_MULTIPLICITY, 2)
    if not relooked:
        assert got.row == min(old, new) and got.value - got.expected == (1 if new < old else -1)
    m = c.multiplicities.copy()
    m[0, 9] += 1
    got = agree(s, multiplicities=m)
    assert (got.kind, got.row, got.expected - got.value) == (binding.UNSAT_MULTIPLICITY, 9, 1)
    m = c.multiplicities.copy()
    m[0, 9] -= 1
    m[0, n - 1] += 1                                   # moved onto a padding row
    got = agree(s, multiplicities=m)
    assert (got.kind, got.row, got.failures[4]) == (binding.UNSAT_MULTIPLICITY, 9, 2)
    m = c.multiplicities.copy()
    m[0, n - 1] += 1                                   # the padding class alone: named by its first row
    got = agree(s, multiplicities=m)
    assert (got.kind, got.row, got.value, got.expected) == (binding.UNSAT_MULTIPLICITY, c.total_tables_len, 0, 1)
    if relooked:                                       # rows 0 and relooked - 1 are equal: only the sum of their multiplicities counts
        m = c.multiplicities.copy()
        m[0, relooked - 1], m[0, 0] = m[0, relooked - 1] + m[0, 0], 0
        assert agree(s, multiplicities=m).kind == binding.SAT


@pytest.mark.parametrize("name", ["seams10", "golden10", "tidvar13"])
def test_noncanonical_cells_give_the_same_report(name):
    s = setup(name)
    c = s.circuit
    gi = K.gate_index(c, "ReductionGate<4>")
    full, _ = K.plant_gate(c, gi, int(K.gate_rows(c, gi)[-1]))
    for w in (K.full_witness(c), full, K.plant_lookup_miss(c, 7, 2)):
        nc = K.noncanonical(w)
        assert np.any(nc != w)
        agree(s, nc, K.noncanonical(c.multiplicities), want=R.check(c, w))


def test_from_dumps():
    from era_boojum_amd import memcopy_format as M
    s = setup("witness10")
    c = s.circuit
    V, n, Wc = c.num_vars, c.n, c.num_witness_cols
    all_values = np.concatenate([c.variables.reshape(-1), c.witness.reshape(-1)])
    var_ids = np.arange(V * n, dtype=np.int64).reshape(V, n)
    wit_ids = V * n + np.arange(Wc * n, dtype=np.int64).reshape(Wc, n)
    pubs = [(col, row) for col, row, _ in c.public_inputs]
    mult = c.multiplicities[0, :c.total_tables_len].astype(np.uint32)
    hints = (M.write_variables_hint(var_ids), M.write_variables_hint(wit_ids))
    got = s.check_satisfied_from_dumps(M.write_witness_vec(pubs, all_values, mult), *hints)
    assert got.kind == binding.SAT and got.failures == (0, 0, 0, 0, 0)
    gi = K.gate_index(c, "ZeroCheckGate[witness]")
    row = int(K.gate_rows(c, gi)[3])
    cell = V + (c.gates[gi].reps - 1) * c.gates[gi].wit_stride          # the inverse in the last repetition's witness column
    broken = all_values.copy()
    broken[cell * n + row] = (int(broken[cell * n + row]) + 1) % E.P
    got = s.check_satisfied_from_dumps(M.write_witness_vec(pubs, broken, mult), *hints)
    cols = agree(s, broken.reshape(V + Wc, n))
    assert got == cols and got.kind == binding.UNSAT_GATE and got.row == row
    with pytest.raises(E.BoojumHipError, match="invalid.*bj_check_satisfied_from_dumps: null argument"):
        s.check_satisfied_from_dumps(M.write_witness_vec(pubs, all_values, mult), None, hints[1])


def _neutral(s, c, bad):
    """prove, check (satisfied), check (broken), prove: the same proof, the inputs untouched."""
    c_ = s._ctx
    good = K.full_witness(c)
    d_good, d_bad, d_m = c_.upload(good), c_.upload(bad), c_.upload(c.multiplicities)
    try:
        before, _ = s.prove_dev(d_good, d_m)
        assert s.check_satisfied_dev(d_good, d_m).kind == binding.SAT
        rep = s.check_satisfied_dev(d_bad, d_m)
        after, _ = s.prove_dev(d_good, d_m)
        assert np.array_equal(before, after)
        assert np.array_equal(c_.d2h(d_good, good.shape), good) and np.array_equal(c_.d2h(d_bad, bad.shape), bad)
        assert np.array_equal(c_.d2h(d_m, c.multiplicities.shape), c.multiplicities)
        return rep, before
    finally:
        for p in (d_good, d_bad, d_m):
            c_.free(p)


def test_a_check_does_not_disturb_proofs():
    s = setup("spec10")
    c = s.circuit
    bad, _ = K.plant_specialized(c, 1, 5)
    rep, _ = _neutral(s, c, bad)
    assert rep.kind == binding.UNSAT_SPECIALIZED_GATE and rep.row == 5


def test_a_check_on_a_sharded_setup():
    """Both ranks of a two-way sharded setup (threads of this process, binding.ThreadGroup): same reports, same proofs."""
    c = K.circuit("tidvar13")
    bad = K.plant_lookup_miss(c, 4000, 5)
    single, _ = setup("tidvar13").prove()
    group, out, errors = E.ThreadGroup(2), [None, None], []

    def rank(r):
        try:
            cx = E.Context(0)
            s = E.ProverSetup(cx, c, 8, 16, 30, comm=group.comm(cx, r))
            out[r] = _neutral(s, c, bad)
            s.close()
            cx.close()
        except BaseException as e:      # noqa: BLE001 — reported by the main thread
            errors.append(e)
            group._barrier.abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    want = R.check(c, bad)
    for rep, proof in out:
        assert (rep.kind, rep.gate, rep.row, rep.failures) == (want.kind, want.gate, want.row, want.failures)
        assert np.array_equal(proof, single)


def test_argument_errors():
    s = setup("sha10")
    c = s.circuit
    lib, h = s._lib, s._ctx._h
    d_v, d_m = ctx().upload(c.variables), ctx().upload(c.multiplicities)
    rep = binding._UnsatReport()
    try:
        assert lib.bj_check_satisfied(h, s._h, d_v, d_m, None) == -1
        assert lib.bj_check_satisfied(h, s._h, None, d_m, C.byref(rep)) == -1
        assert lib.bj_check_satisfied(h, None, d_v, d_m, C.byref(rep)) == -1
        assert lib.bj_check_satisfied(h, s._h, d_v, None, C.byref(rep)) == -1
        assert b"multiplicities required" in lib.bj_last_error(h)
        assert lib.bj_check_satisfied(h, s._h, d_v, d_m, C.byref(rep)) == 0 and rep.kind == 0
    finally:
        ctx().free(d_v)
        ctx().free(d_m)
