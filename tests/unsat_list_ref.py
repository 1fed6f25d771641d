"""Exact NumPy restatement of bj_list_unsatisfied (include/boojum_hip.h) for an era_boojum_amd.synthetic.Circuit: the COMPLETE
list of failures in the order satisfiability_ref.py documents for the first one, carried through to the end, and the totals per
kind.  Gate terms come from satisfiability_ref._gate_terms; the lookup and class rules of satisfiability_ref.check are restated
here so that every miss and every wrong class is kept, not the first.  No random combination.

An entry is the tuple (kind, gate, repetition, term, row, value, expected) of bj_unsat_entry."""
import numpy as np

import satisfiability_ref as R

P = R.P


def _nonzero_terms(kind, per_gate):
    """per_gate: [(gate index, rows, [rep][term] arrays)] -> entries of `kind`, sorted by (row, gate, repetition, term)."""
    found = []
    for gi, rows, terms in per_gate:
        for r, ts in enumerate(terms):
            for t, v in enumerate(ts):
                for i in np.flatnonzero(v):
                    found.append((int(rows[i]), gi, r, t, int(v[i])))
    found.sort()
    return [(kind, gi, r, t, row, value, 0) for row, gi, r, t, value in found]


def listing(c, variables=None, multiplicities=None, witness=None):
    """(entries, totals): every entry of circuit `c` with the given witness (defaults: the circuit's own columns), and
    totals[k] = entries of kind k, totals[0] their sum."""
    n = c.n
    var = R._canon(c.variables if variables is None else variables)
    wit = c.witness if witness is None else witness
    if var.shape[0] == c.num_vars + c.num_witness_cols and c.num_witness_cols:
        var, wit = var[:c.num_vars], var[c.num_vars:]
    wit = R._canon(wit) if wit is not None else None
    consts = R._canon(c.constants)
    entries = []

    # 1: general-purpose gates on the rows their selector path picks (one gate per row: the order is (row, repetition, term))
    per_gate = []
    for gi, g in enumerate(c.gates):
        m = np.ones(n, dtype=bool)
        for i, bit in enumerate(g.path):
            m &= consts[i] == (1 if bit else 0)
        rows = np.flatnonzero(m)
        if rows.size and g.num_terms:
            per_gate.append((gi, rows, R._gate_terms(c, g, rows, var, consts, wit)))
    entries += _nonzero_terms(R.UNSAT_GATE, per_gate)

    # 2: gates over specialized columns, every row
    col = c.num_gp_vars + c.num_lookup_vars
    ccol = c.num_constant_cols - sum(g.reps * g.const_stride for g in c.specialized_gates)
    per_gate, all_rows = [], np.arange(n)
    for gi, g in enumerate(c.specialized_gates):
        terms = []
        for r in range(g.reps):
            ccols = [consts[ccol + r * g.const_stride + k] for k in range(g.const_stride)]
            terms.append(g.program.evaluate_columns(list(var[col + r * g.var_stride: col + (r + 1) * g.var_stride]), ccols))
        per_gate.append((gi, all_rows, terms))
        col += g.reps * g.var_stride
        ccol += g.reps * g.const_stride
    entries += _nonzero_terms(R.UNSAT_SPECIALIZED_GATE, per_gate)

    # 3, 4: lookups — classes of equal table rows named by their smallest row
    if c.lookup_reps:
        mult = R._canon(c.multiplicities if multiplicities is None else multiplicities).reshape(-1)
        tab = R._canon(c.tables)
        rep_of, classes = {}, np.empty(n, dtype=np.int64)
        for r, key in enumerate(map(tuple, tab.T.tolist())):
            classes[r] = rep_of.setdefault(key, r)
        count = np.zeros(n, dtype=object)
        cps, w = c.lookup_cols_per_sub, c.lookup_width
        misses = []
        for sub in range(c.lookup_reps):
            cols = [var[c.num_gp_vars + sub * cps + j] for j in range(w)]
            cols.append(var[c.num_gp_vars + sub * cps + w] if c.table_id_as_variable else consts[c.table_id_col])
            for row, key in enumerate(map(tuple, np.stack(cols).T.tolist())):
                r = rep_of.get(key)
                if r is None:
                    misses.append((row, sub))
                else:
                    count[r] += 1
        entries += [(R.UNSAT_LOOKUP, sub, 0, 0, row, 0, 0) for row, sub in sorted(misses)]
        expected = np.zeros(n, dtype=object)
        for r in range(n):
            if mult[r]:
                expected[classes[r]] += int(mult[r])
        entries += [(R.UNSAT_MULTIPLICITY, 0, 0, 0, r, int(count[r]), int(expected[r] % P))
                    for r in sorted(set(rep_of.values())) if expected[r] % P != count[r]]

    totals = [0] * 5
    for e in entries:
        totals[e[0]] += 1
    totals[0] = len(entries)
    return entries, tuple(totals)
