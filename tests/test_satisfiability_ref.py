"""CPU: the exact restatement of bj_check_satisfied (tests/satisfiability_ref.py) says BJ_SAT exactly where
synthetic.check_satisfied passes and names the planted cell on tampered witnesses of every geometry the GPU test uses."""
import numpy as np
import pytest

from era_boojum_amd import synthetic as S

import satisfiability_cases as K
import satisfiability_ref as R


@pytest.mark.parametrize("name", ["seams10", "sha10", "tidvar13", "golden10", "poseidon1", "extended10", "jit10", "witness10", "spec10", "real_sha"])
def test_satisfied_circuits_are_sat(name):
    c = K.circuit(name)
    assert S.check_satisfied(c)
    rep = R.check(c)
    assert rep.fields() == R.Report().fields()


# (geometry, gate name, row or None = the gate's last row)
GATE_CASES = [("seams10", "ConstantsAllocatorGate", 0), ("seams10", "FmaGateInBaseFieldWithoutConstant", 255),
              ("seams10", "FmaGateInBaseFieldWithoutConstant", 256), ("seams10", "ReductionGate<4>", 1023),
              ("extended10", "UIntXAddGate", None), ("jit10", "MatrixMultiplicationGate[host]", None),
              ("golden10", "Poseidon2FlattenedGate", None), ("poseidon1", "PoseidonFlattenedGate", None),
              ("witness10", "ZeroCheckGate[witness]", None)]


@pytest.mark.parametrize("name,gate,row", GATE_CASES)
def test_planted_gate_failure_is_named(name, gate, row):
    c = K.circuit(name)
    gi = K.gate_index(c, gate)
    row = int(K.gate_rows(c, gi)[-1]) if row is None else row
    full, (g, r, t) = K.plant_gate(c, gi, row)
    rep = R.check(c, full)
    assert (rep.kind, rep.gate, rep.repetition, rep.term, rep.row) == (R.UNSAT_GATE, g, r, t, row)
    assert rep.value != 0 and rep.failures == (0, 1, 0, 0, 0)
    assert r == c.gates[gi].reps - 1
    with pytest.raises(AssertionError, match="unsatisfied"):
        S.check_satisfied(_with(c, full))


def _with(c, full):
    import dataclasses
    return dataclasses.replace(c, variables=full[:c.num_vars], witness=full[c.num_vars:] if c.num_witness_cols else None)


def test_two_failures_and_both_gate_kinds():
    c = K.circuit("seams10")
    fma = K.gate_index(c, "FmaGateInBaseFieldWithoutConstant")
    full, _ = K.plant_gate(c, fma, 300)
    full, (g, r, t) = K.plant_gate(c, fma, 256, full)
    rep = R.check(c, full)
    assert (rep.kind, rep.row, rep.gate, rep.repetition, rep.term, rep.failures[1]) == (R.UNSAT_GATE, 256, g, r, t, 2)
    s = K.circuit("spec10")
    full, where = K.plant_specialized(s, 1, s.n - 1)
    rep = R.check(s, full)
    assert (rep.kind, rep.row, (rep.gate, rep.repetition, rep.term), rep.failures) == (R.UNSAT_SPECIALIZED_GATE, s.n - 1, where, (0, 0, 1, 0, 0))
    full, _ = K.plant_gate(s, K.gate_index(s, "ReductionGate<4>"), int(K.gate_rows(s, K.gate_index(s, "ReductionGate<4>"))[0]), full)
    rep = R.check(s, full)
    assert rep.kind == R.UNSAT_GATE and rep.failures == (0, 1, 1, 0, 0)


@pytest.mark.parametrize("name", ["sha10", "tidvar13"])
def test_lookup_failures_are_named(name):
    c = K.circuit(name)
    n, last = c.n, c.lookup_reps - 1
    for row, sub in ((5, 0), (n - 1, last)):
        rep = R.check(c, K.plant_lookup_miss(c, row, sub))
        assert (rep.kind, rep.row, rep.gate, rep.failures) == (R.UNSAT_LOOKUP, row, sub, (0, 0, 0, 1, 1))   # its table row is now over-counted too
    full, (old, new) = K.plant_lookup_swap(c, 77, 3)
    rep = R.check(c, full)
    assert (rep.kind, rep.row, rep.failures) == (R.UNSAT_MULTIPLICITY, min(old, new), (0, 0, 0, 0, 2))
    assert rep.value - rep.expected == (1 if new < old else -1)
    m = c.multiplicities.copy()
    m[0, 9] += 1
    rep = R.check(c, multiplicities=m)
    assert (rep.kind, rep.row, rep.expected - rep.value, rep.failures[4]) == (R.UNSAT_MULTIPLICITY, 9, 1, 1)
    m = c.multiplicities.copy()
    m[0, n - 1] += 1                                   # onto a padding row: the padding class is named by its first row
    rep = R.check(c, multiplicities=m)
    assert (rep.kind, rep.row, rep.value, rep.expected) == (R.UNSAT_MULTIPLICITY, c.total_tables_len, 0, 1)


@pytest.mark.parametrize("rows", [16, 1021])
def test_other_tables_and_noncanonical_cells(rows):
    c = K.relooked("sha10", rows)
    assert R.check(c).fields() == R.Report().fields()
    m = c.multiplicities.copy()
    m[0, rows - 1], m[0, 0] = m[0, rows - 1] + m[0, 0], 0        # rows 0 and rows - 1 are one class: only their sum counts
    assert R.check(c, multiplicities=m).kind == R.SAT
    full = K.plant_lookup_miss(c, 3, 1)
    assert R.check(c, K.noncanonical(full)).fields() == R.check(c, full).fields()
    assert np.any(K.noncanonical(full) != full)
