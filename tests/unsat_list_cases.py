"""Planted witnesses shared by test_unsat_list_ref.py (CPU) and test_gpu_list_unsatisfied.py (GPU), on the circuits of
satisfiability_cases.py.  A case is (circuit name, full witness, multiplicities); every case and its reference listing
(unsat_list_ref.listing) is built once per session and never modified."""
import functools

import numpy as np

import satisfiability_cases as K
import unsat_list_ref as L

EDGE_ROWS = (0, 63, 64, 255, 256, 511, 512, -1)     # wave and block edges of the compaction, and the last row (n - 1)


def _plant_edge(c, row, full):
    """One wrong cell on `row`: in the gate the row selects — or, where that is NopGate (no term can fail: rows 511 and 512 of
    seams10), in the first lookup sub-argument, which the same compaction lists as kind 3."""
    gi = [g for g in range(len(c.gates)) if row in K.gate_rows(c, g)][0]
    if c.gates[gi].num_terms == 0:
        return K.plant_lookup_miss(c, row, 0, full)
    return K.plant_gate(c, gi, row, full)[0]


def _edges(which):
    c = K.circuit("seams10")
    full = K.full_witness(c)
    for row in (EDGE_ROWS if which is None else (which,)):
        full = _plant_edge(c, row % c.n, full)
    return "seams10", full, c.multiplicities


def _dense():
    """General-purpose variable column 0 of sha10 changed on every row: every row whose gate reads it fails."""
    c = K.circuit("sha10")
    full = K.full_witness(c)
    full[0] = (full[0] + np.uint64(1)) % np.uint64(K.P)
    return "sha10", full, c.multiplicities


def _mixed(name):
    """A general-purpose gate failure, specialized-gate failures on two rows, two missing tuples in different sub-arguments of
    one row, one wrong multiplicity."""
    c = K.circuit(name)
    red = K.gate_index(c, "ReductionGate<4>")
    full, _ = K.plant_gate(c, red, int(K.gate_rows(c, red)[7]))
    full, _ = K.plant_specialized(c, 0, 5, full)
    full, _ = K.plant_specialized(c, len(c.specialized_gates) - 1, c.n - 1, full)
    full = K.plant_lookup_miss(c, 300, 1, full)
    full = K.plant_lookup_miss(c, 300, 6, full)
    m = c.multiplicities.copy()
    m[0, 9] += 1
    return name, full, m


def _poseidon_row():
    """One input cell of a Poseidon2 row of golden10: many of the row's 118 terms are non-zero."""
    c = K.circuit("golden10")
    gi = K.gate_index(c, "Poseidon2FlattenedGate")
    full = K.full_witness(c)
    row = int(K.gate_rows(c, gi)[64])
    full[0, row] = (int(full[0, row]) + 1) % K.P
    return "golden10", full, c.multiplicities


CASES = {"edges": lambda: _edges(None), "dense": _dense, "mixed_spec10": lambda: _mixed("spec10"), "mixed_tidvar13": lambda: _mixed("tidvar13"),
         "poseidon_row": _poseidon_row}
CASES.update({"edge_%d" % i: (lambda r=r: _edges(r)) for i, r in enumerate(EDGE_ROWS)})
PLANTED = sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(entries, totals) of the restatement for case `name`."""
    cname, full, mult = case(name)
    return L.listing(K.circuit(cname), full, mult)
