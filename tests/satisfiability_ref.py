"""Exact NumPy restatement of bj_check_satisfied (include/boojum_hip.h) for an era_boojum_amd.synthetic.Circuit: every term of
every gate on its rows (the hand-written kinds as formulas, every other evaluator through GateProgram.evaluate_columns), every
looked-up tuple against the table rows, every class of equal table rows against its multiplicities.  No random combination:
this is what the GPU report is compared with, field by field.

The order that defines the first failure is the reference's (satisfiability_test.rs:15-353) extended to lookups:
  1  gates over general-purpose columns: ascending row, the selected gate, ascending repetition, ascending term
  2  gates over specialized columns: ascending row, gate in declaration order, repetition, term
  3  lookups: ascending row, then sub-argument
  4  multiplicities: ascending representative (smallest row) of a class of equal table rows
Copy constraints are not part of it."""
from dataclasses import dataclass

import numpy as np

from era_boojum_amd import field_np as F
from era_boojum_amd import synthetic as S

P = F.P
SAT, UNSAT_GATE, UNSAT_SPECIALIZED_GATE, UNSAT_LOOKUP, UNSAT_MULTIPLICITY = range(5)


@dataclass
class Report:
    kind: int = SAT
    gate: int = 0
    repetition: int = 0
    term: int = 0
    row: int = 0
    value: int = 0
    expected: int = 0
    failures: tuple = (0, 0, 0, 0, 0)

    def fields(self):
        return (self.kind, self.gate, self.repetition, self.term, self.row, self.value, self.expected, tuple(self.failures))


def _canon(a):
    return F.canon(np.ascontiguousarray(a, dtype=np.uint64))


def _gate_terms(c, g, rows, var, consts, wit):
    """[repetition][term] -> values on `rows` for a gate over general-purpose columns."""
    d = len(g.path)
    out = []
    for r in range(g.reps):
        b = r * g.var_stride
        if g.kind == S.GATE_CONSTANT_ALLOCATOR:
            terms = [F.sub(var[b][rows], consts[d + r * g.const_stride][rows])]
        elif g.kind == S.GATE_FMA:
            terms = [F.sub(F.add(F.mul(consts[d][rows], F.mul(var[b][rows], var[b + 1][rows])), F.mul(consts[d + 1][rows], var[b + 2][rows])),
                           var[b + 3][rows])]
        elif g.kind == S.GATE_REDUCTION4:
            acc = np.zeros(len(rows), dtype=np.uint64)
            for i in range(4):
                acc = F.add(acc, F.mul(var[b + i][rows], consts[d + i][rows]))
            terms = [F.sub(acc, var[b + 4][rows])]
        elif g.kind == S.GATE_NOP:
            terms = []
        else:
            prog = g.program
            if prog is None:
                from era_boojum_amd.gate_program import poseidon2_flattened_compact_program
                prog = poseidon2_flattened_compact_program()
            vcols = [var[b + k][rows] for k in range(g.principal_width)]
            ccols = [consts[k][rows] for k in range(d + r * g.const_stride, consts.shape[0])]
            wcols = [wit[k][rows] for k in range(r * g.wit_stride, wit.shape[0])] if wit is not None else []
            terms = prog.evaluate_columns(vcols, ccols, wcols)
        assert len(terms) == g.num_terms, (g.name, len(terms), g.num_terms)
        out.append(terms)
    return out


def _first_nonzero(per_gate, n):
    """per_gate: [(gate index, rows, [rep][term] arrays)] -> (failing rows as a set-like bool array, best (row, gate, rep, term, value))."""
    bad = np.zeros(n, dtype=bool)
    best = None
    for gi, rows, terms in per_gate:
        for r, ts in enumerate(terms):
            for t, v in enumerate(ts):
                nz = np.flatnonzero(v)
                if nz.size == 0:
                    continue
                bad[rows[nz]] = True
                cand = (int(rows[nz[0]]), gi, r, t, int(v[nz[0]]))
                if best is None or cand[:4] < best[:4]:
                    best = cand
    return bad, best


def check(c, variables=None, multiplicities=None, witness=None):
    """The full report for circuit `c` with the given witness (defaults: the circuit's own columns)."""
    n = c.n
    var = _canon(c.variables if variables is None else variables)
    wit = c.witness if witness is None else witness
    if var.shape[0] == c.num_vars + c.num_witness_cols and c.num_witness_cols:
        var, wit = var[:c.num_vars], var[c.num_vars:]
    wit = _canon(wit) if wit is not None else None
    consts = _canon(c.constants)
    failures = [0, 0, 0, 0, 0]
    firsts = {}

    # 1: general-purpose gates on the rows their selector path picks
    per_gate = []
    for gi, g in enumerate(c.gates):
        m = np.ones(n, dtype=bool)
        for i, bit in enumerate(g.path):
            m &= consts[i] == (1 if bit else 0)
        rows = np.flatnonzero(m)
        if rows.size and g.num_terms:
            per_gate.append((gi, rows, _gate_terms(c, g, rows, var, consts, wit)))
    bad, best = _first_nonzero(per_gate, n)
    failures[1] = int(bad.sum())
    if best:
        firsts[UNSAT_GATE] = Report(UNSAT_GATE, best[1], best[2], best[3], best[0], best[4])

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
    bad, best = _first_nonzero(per_gate, n)
    failures[2] = int(bad.sum())
    if best:
        firsts[UNSAT_SPECIALIZED_GATE] = Report(UNSAT_SPECIALIZED_GATE, best[1], best[2], best[3], best[0], best[4])

    # 3, 4: lookups
    if c.lookup_reps:
        mult = _canon(c.multiplicities if multiplicities is None else multiplicities).reshape(-1)
        tab = _canon(c.tables)
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
        failures[3] = len(misses)
        if misses:
            row, sub = min(misses)
            firsts[UNSAT_LOOKUP] = Report(UNSAT_LOOKUP, sub, 0, 0, row)
        expected = np.zeros(n, dtype=object)
        for r in range(n):
            if mult[r]:
                expected[classes[r]] += int(mult[r])
        wrong = [r for r in sorted(set(rep_of.values())) if expected[r] % P != count[r]]
        failures[4] = len(wrong)
        if wrong:
            r = wrong[0]
            firsts[UNSAT_MULTIPLICITY] = Report(UNSAT_MULTIPLICITY, 0, 0, 0, r, int(count[r]), int(expected[r] % P))

    rep = firsts[min(firsts)] if firsts else Report()
    rep.failures = tuple(failures)
    return rep
