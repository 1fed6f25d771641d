"""CPU: the restatement of bj_list_unsatisfied (tests/unsat_list_ref.py) against the restatement of bj_check_satisfied
(tests/satisfiability_ref.py) on every planted case of unsat_list_cases.py — its first entry is that report, its totals of kinds 3
and 4 are that report's failures, the distinct rows among its entries of kinds 1 and 2 are that report's failing rows — and the
order the header documents."""
import pytest

import satisfiability_cases as K
import satisfiability_ref as R
import unsat_list_cases as U
import unsat_list_ref as L


@pytest.mark.parametrize("name", ["sha10", "seams10", "spec10", "golden10"])
def test_satisfied_circuits_list_nothing(name):
    assert L.listing(K.circuit(name)) == ([], (0, 0, 0, 0, 0))


@pytest.mark.parametrize("name", U.PLANTED)
def test_listing_agrees_with_the_report(name):
    cname, full, mult = U.case(name)
    entries, totals = U.reference(name)
    rep = R.check(K.circuit(cname), full, mult)
    assert entries and entries[0] == rep.fields()[:7]
    assert totals[3] == rep.failures[3] and totals[4] == rep.failures[4]
    for kind in (1, 2):
        assert len({e[4] for e in entries if e[0] == kind}) == rep.failures[kind]
    assert totals[0] == len(entries) == sum(totals[1:])
    # kinds ascending; inside a kind (row, gate, repetition, term) ascending and no entry twice
    keys = [(e[0], e[4], e[1], e[2], e[3]) for e in entries]
    assert keys == sorted(set(keys))
    assert all(e[5] != 0 for e in entries if e[0] in (1, 2)) and all(e[5] != e[6] for e in entries if e[0] == 4)


def test_the_cases_cover_what_they_are_meant_to():
    n = K.circuit("seams10").n
    entries, totals = U.reference("edges")
    assert sorted({e[4] for e in entries if e[0] in (1, 3)}) == sorted(r % n for r in U.EDGE_ROWS)
    _, totals = U.reference("dense")
    assert totals[1] > 512 and totals[1] == totals[0]               # more flagged rows than one block, than the small capacities
    for name in ("mixed_spec10", "mixed_tidvar13"):
        _, totals = U.reference(name)
        assert totals[1] >= 1 and totals[2] >= 2 and totals[3] == 2 and totals[4] >= 1
    entries, totals = U.reference("poseidon_row")
    assert totals[1] > 8 and len({e[4] for e in entries}) == 1      # many terms of one row
