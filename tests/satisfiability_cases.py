"""Circuits and tampered witnesses shared by test_satisfiability_ref.py (CPU) and test_gpu_check_satisfied.py (GPU).  Every
circuit is built once per session (functools.lru_cache) and never modified: tampering works on copies of the columns."""
import dataclasses
import functools

import numpy as np

from era_boojum_amd import field_np as F
from era_boojum_amd import synthetic as S

import satisfiability_ref as R

P = F.P


def _seams_gates():
    """The bench's four gates with NopGate third, so that ReductionGate<4> owns the rows up to n - 1."""
    g = S.sha_bench_gates()
    return [g[0], g[1], g[3], g[2]]


GEOMETRIES = {
    # name: builder.  2^10 rows: ConstantsAllocator rows 0..50, FMA 51..510 (the reduction's block seam 255 | 256), Nop, Reduction 613..1023
    "seams10": lambda: S.sha_shaped_circuit(10, seed=3, table_bits=2, gates=_seams_gates(), mix=(0.05, 0.45, 0.1)),
    "sha10": lambda: S.sha_shaped_circuit(10, seed=11, table_bits=2),
    "sha13": lambda: S.sha_shaped_circuit(13, seed=12, table_bits=3),
    "real_sha": lambda: _real_sha()[0],
    "tidvar13": lambda: S.sha_shaped_circuit(13, seed=7, table_bits=2, table_id_as_variable=True, boolean_columns=2),
    "golden10": lambda: S.recursion_like_circuit(10, seed=4),
    "poseidon1": lambda: S.recursion_like_circuit(9, seed=41, poseidon1="kind"),
    "extended10": lambda: S.sha_shaped_circuit(10, seed=13, table_bits=2, extended=True),
    "jit10": lambda: S.sha_shaped_circuit(10, seed=14, table_bits=2, gates=S.host_gates(), mix=(0.05, 0.3, 0.3, 0.2)),
    "witness10": lambda: S.sha_shaped_circuit(10, seed=5, table_bits=2, gates=S.witness_gates(60, 4, 5), mix=(0.05, 0.3, 0.3, 0.2),
                                              num_witness_cols=5),
    "spec10": lambda: S.sha_shaped_circuit(10, seed=33, table_bits=2, boolean_columns=2, specialized_constant_columns=3),
    "sha16": lambda: S.sha_shaped_circuit(16, seed=16, table_bits=2, gates=_seams_gates(), mix=(0.05, 0.45, 0.1)),
}
SATISFIED = ["sha10", "sha13", "real_sha", "tidvar13", "golden10", "poseidon1", "witness10", "jit10"]


@functools.lru_cache(maxsize=None)
def _real_sha():
    from era_boojum_amd import sha256_circuit as SHA
    return SHA.sha256_circuit(SHA.bench_message(33, seed=3), return_info=True)


@functools.lru_cache(maxsize=None)
def circuit(name):
    return GEOMETRIES[name]()


def full_witness(c, variables=None, witness=None):
    """[num_vars + num_witness_cols][n] as the entry points take it."""
    v = np.array(c.variables if variables is None else variables, dtype=np.uint64)
    w = c.witness if witness is None else witness
    return v if w is None else np.concatenate([v, np.asarray(w, dtype=np.uint64)], axis=0)


def gate_index(c, name):
    return [g.name for g in c.gates].index(name)


def gate_rows(c, gi):
    m = np.ones(c.n, dtype=bool)
    for i, bit in enumerate(c.gates[gi].path):
        m &= c.constants[i] == (1 if bit else 0)
    return np.flatnonzero(m)


def plant_gate(c, gi, row, full=None):
    """A copy of the full witness with ONE cell of the last repetition of gate `gi` changed on `row`, chosen so that the first
    non-zero term of that repetition is its last one where such a cell exists.  Returns (witness, (gate, repetition, term))."""
    g = c.gates[gi]
    full = full_witness(c) if full is None else full.copy()
    V, rep = c.num_vars, g.reps - 1
    cells = [rep * g.var_stride + k for k in range(g.principal_width)] + [V + rep * g.wit_stride + k for k in range(g.wit_stride)]
    consts = F.canon(np.ascontiguousarray(c.constants))
    rows = np.array([row])
    found = None
    order = list(reversed(cells))
    if "Poseidon" in g.name:                      # the flattened permutations: the last term is the last output cell's (variable 23)
        order.insert(0, 23)
    for cell in order:
        trial = full.copy()
        trial[cell, row] = (int(trial[cell, row]) + 1) % P
        var, wit = F.canon(trial[:V]), (F.canon(trial[V:]) if c.num_witness_cols else None)
        terms = R._gate_terms(c, g, rows, var, consts, wit)
        nz = [(r, t) for r in range(g.reps) for t in range(g.num_terms) if int(terms[r][t][0])]
        if nz and nz[0][0] == rep:
            if found is None:
                found = (trial, (gi, rep, nz[0][1]))
            if nz[0][1] == g.num_terms - 1:
                return trial, (gi, rep, nz[0][1])
    assert found is not None, "no cell of %s changes its last repetition" % g.name
    return found


def plant_specialized(c, si, row, full=None):
    """One cell of the last repetition of specialized gate `si` changed on `row`."""
    full = full_witness(c) if full is None else full.copy()
    col = c.num_gp_vars + c.num_lookup_vars + sum(g.reps * g.var_stride for g in c.specialized_gates[:si])
    g = c.specialized_gates[si]
    cell = col + (g.reps - 1) * g.var_stride
    full[cell, row] = (int(full[cell, row]) + 2) % P          # a bit + 2 is no bit; a constant + 2 is not the constant
    return full, (si, g.reps - 1, g.num_terms - 1)


def lookup_cell(c, sub, j):
    return c.num_gp_vars + sub * c.lookup_cols_per_sub + j


def plant_lookup_miss(c, row, sub, full=None):
    full = full_witness(c) if full is None else full.copy()
    full[lookup_cell(c, sub, 0), row] = np.uint64(0x1234567)  # no table holds a limb this large
    return full


def table_row_of(c, full, row, sub):
    key = [int(full[lookup_cell(c, sub, j), row]) for j in range(c.lookup_width)]
    key.append(int(full[lookup_cell(c, sub, c.lookup_width), row]) if c.table_id_as_variable else int(c.constants[c.table_id_col, row]))
    hits = np.flatnonzero(np.all(c.tables == np.array(key, dtype=np.uint64)[:, None], axis=0))
    return int(hits[0])


def plant_lookup_swap(c, row, sub, full=None):
    """The tuple at (row, sub) changed into another row of the same table.  Returns (witness, the two table rows)."""
    full = full_witness(c) if full is None else full.copy()
    old = table_row_of(c, full, row, sub)
    tid = c.tables[c.lookup_width, old]
    same = np.flatnonzero(c.tables[c.lookup_width] == tid)
    new = int(same[0]) if int(same[0]) != old else int(same[1])
    if np.array_equal(c.tables[:, new], c.tables[:, old]):     # an equal row would be the same class
        new = int([r for r in same if not np.array_equal(c.tables[:, r], c.tables[:, old])][0])
    for j in range(c.lookup_width):
        full[lookup_cell(c, sub, j), row] = c.tables[j, new]
    return full, (old, new)


def noncanonical(a):
    """p added to every cell that can take it in 64 bits."""
    a = np.array(a, dtype=np.uint64)
    return np.where(a < np.uint64((1 << 32) - 1), a + np.uint64(P), a)


@functools.lru_cache(maxsize=None)
def relooked(name, table_rows, seed=1):
    """Circuit `name` with another lookup table: table_rows rows of random words under table id 1, the last row a duplicate of
    row 0 (a class of two), every sub-argument of every row looking one of them up; padding rows all zero."""
    c = circuit(name)
    n, w, T = c.n, c.lookup_width, table_rows
    rng = np.random.default_rng(seed)
    tables = np.zeros((w + 1, n), dtype=np.uint64)
    tables[:w, :T] = rng.integers(0, P, size=(w, T), dtype=np.uint64)
    tables[w, :T] = 1
    tables[:, T - 1] = tables[:, 0]
    variables, constants = c.variables.copy(), c.constants.copy()
    if not c.table_id_as_variable:
        constants[c.table_id_col] = 1
    mult = np.zeros(n, dtype=np.uint64)
    for sub in range(c.lookup_reps):
        pick = rng.integers(0, T, size=n)
        for j in range(w):
            variables[lookup_cell(c, sub, j)] = tables[j][pick]
        if c.table_id_as_variable:
            variables[lookup_cell(c, sub, w)] = 1
        mult += np.bincount(pick, minlength=n).astype(np.uint64)
    return dataclasses.replace(c, variables=variables, constants=constants, tables=tables, multiplicities=mult.reshape(1, n),
                               total_tables_len=T)
