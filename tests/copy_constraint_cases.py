"""Inputs and the numpy restatement shared by test_gpu_copy_constraints.py and its sharded worker.  Nothing here touches the GPU:
identities come from field_np, sigma from sha256_circuit.sigma_from_placement (numpy path), the cell a sigma word names from
np.searchsorted over the sorted identities."""
import dataclasses
import functools

import numpy as np

from era_boojum_amd import field_np as F
from era_boojum_amd import sha256_circuit as SHA
from era_boojum_amd import synthetic as S

P = F.P
NO_CELL = 0xFFFFFFFF
MAX_INDEX = (1 << 32) - 2


def identities(V, log_n, ks):
    om = F.powers(F.omega(log_n), 1 << log_n)
    return np.stack([F.mul(om, np.uint64(k)) for k in ks[:V]])


def sigma_from_placement(var_ids, log_n, ks):
    """The numpy path of the comparator (the native walk indexes int32 tables: no indices up to 2^32 - 2)."""
    sig = identities(var_ids.shape[0], log_n, ks)
    saved, F._NATIVE = F._NATIVE, None
    try:
        SHA.sigma_from_placement(var_ids, int(var_ids.max()) + 1, sig)
    finally:
        F._NATIVE = saved
    return sig


def expected_cells(sig, log_n, ks):
    """[V][n] u32: the cell column * n + row whose identity each word is (as a residue), NO_CELL where there is none."""
    V = sig.shape[0]
    ids = identities(V, log_n, ks).reshape(-1)
    order = np.argsort(ids, kind="stable")
    words = F.canon(sig).reshape(-1)
    pos = np.minimum(np.searchsorted(ids[order], words), len(ids) - 1)
    hit = ids[order][pos] == words
    return np.where(hit, order[pos], NO_CELL).astype(np.uint32).reshape(sig.shape)


def sparse_placement(log_n, V, seed):
    """[V][n] int64, negative = placeholder, as tests/test_gpu_setup_placement.py makes them: random variables used about three
    times each, 10 % placeholders, indices spread up to 2^32 - 2 by a monotone map; with V >= 3 one variable fills a column and
    one column holds placeholders only."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    k = max(2, V * n // 3)
    v = rng.integers(0, k, size=(V, n), dtype=np.int64)
    v[rng.random((V, n)) < 0.10] = -1
    if V >= 3:
        v[V // 2] = k + 1
        v[V - 1] = -1
    v[0, 0] = v[0, n - 1] = 0            # at least one cycle whatever the draw
    top = int(v.max())
    pool = np.unique(rng.integers(0, MAX_INDEX, size=2 * (top + 1), dtype=np.int64))
    pool = pool[np.sort(rng.choice(len(pool), top + 1, replace=False))]
    pool[-1] = MAX_INDEX
    return np.where(v >= 0, pool[np.maximum(v, 0)], -1)


def keys_of(shape):
    V, n = shape
    return (np.arange(n, dtype=np.int64)[None, :] * V + np.arange(V, dtype=np.int64)[:, None]).reshape(-1)


@dataclasses.dataclass
class Expected:
    kind: int
    column: int = 0
    row: int = 0
    partner_column: int = 0
    partner_row: int = 0
    value: int = 0
    partner_value: int = 0
    variable: int = NO_CELL
    failures: tuple = (0, 0, 0, 0)

    def fields(self):
        return (self.kind, self.column, self.row, self.partner_column, self.partner_row, self.value, self.partner_value, self.variable,
                self.failures)


def check(sig, variables, log_n, ks, var_ids=None):
    """The report bj_check_copy_constraints owes for these sigma and variable columns ([V][n] each)."""
    V, n = sig.shape
    perm = expected_cells(sig, log_n, ks).reshape(-1).astype(np.int64)
    v = F.canon(np.asarray(variables[:V], dtype=np.uint64)).reshape(-1)
    keys = keys_of((V, n))
    valid = perm != NO_CELL
    target = np.where(valid, perm, 0)
    hits = np.bincount(target[valid], minlength=V * n)
    invalid = ~valid
    shared = valid & (hits[target] >= 2)
    differs = valid & (v != v[target])
    failures = (0, int(invalid.sum()), int(valid.sum() - np.count_nonzero(hits)), int(differs.sum()))

    def first(mask):
        cell = int(np.flatnonzero(mask)[np.argmin(keys[mask])])
        return cell, cell // n, cell % n
    if failures[1]:
        _, col, row = first(invalid)
        return Expected(1, col, row, failures=failures)
    if failures[2]:
        cell, col, row = first(shared)
        return Expected(2, col, row, int(perm[cell]) // n, int(perm[cell]) % n, failures=failures)
    if failures[3]:
        cell, col, row = first(differs)
        variable = NO_CELL
        if var_ids is not None:
            variable = int(var_ids[col, row]) if var_ids[col, row] >= 0 else NO_CELL
        return Expected(3, col, row, int(perm[cell]) // n, int(perm[cell]) % n, int(v[cell]), int(v[perm[cell]]), variable, failures)
    return Expected(0, failures=failures)


FIRST, PUBLIC = (0, 0), (3, 5)       # cells the crafted placement puts into cycles; PUBLIC is a public input of the circuit


@functools.lru_cache(maxsize=None)
def free_circuit():
    """A 2^10-row circuit of the bench geometry whose every row selects NopGate, so that no gate constrains a general-purpose cell
    and a changed cell breaks copy constraints ONLY; with a placement crafted over it: random variables over the general-purpose
    columns (the first cell and a public input in cycles of three), and in the last lookup column the cells of equal value
    linked (long cycles through the last cell).  Returns (circuit with that sigma and matching values, var_ids)."""
    c = S.sha_shaped_circuit(10, seed=21, table_bits=2, mix=(0.0, 0.0, 0.0))
    V, n, G = c.num_vars, c.n, c.num_gp_vars
    assert [p[:2] for p in c.public_inputs][0] == PUBLIC
    rng = np.random.default_rng(77)
    var_ids = np.full((V, n), -1, dtype=np.int64)
    k = G * n // 3
    var_ids[:G] = rng.integers(0, k, size=(G, n), dtype=np.int64)
    var_ids[:G][rng.random((G, n)) < 0.10] = -1
    for var, cells in ((k, (FIRST, (7, 100), (20, 1000))), (k + 1, (PUBLIC, (40, 512), (59, n - 1)))):
        for col, row in cells:
            var_ids[col, row] = var
    last = np.asarray(c.variables[V - 1], dtype=np.int64)
    assert int(last.max()) < 1 << 20 and np.count_nonzero(last == last[n - 1]) >= 2
    var_ids[V - 1] = k + 2 + last
    values = rng.integers(0, P, size=int(var_ids[:G].max()) + 1, dtype=np.uint64)
    variables = np.array(c.variables, dtype=np.uint64)
    variables[:G] = np.where(var_ids[:G] >= 0, values[np.maximum(var_ids[:G], 0)], 0)
    sig = sigma_from_placement(var_ids, c.log_n, c.non_residues)
    pubs = [(col, row, int(variables[col, row])) for col, row, _ in c.public_inputs]
    return dataclasses.replace(c, variables=variables, sigmas=sig, public_inputs=pubs), var_ids


def changed(variables, col, row):
    out = np.array(variables, dtype=np.uint64)
    out[col, row] = (int(out[col, row]) + 1) % P
    return out


def moved_last_tuple(c):
    """The last cell sits in a lookup column: the tuple of the last sub-argument on the last row becomes another row of the same
    table whose last word differs, so that the lookup argument holds again once the multiplicities are recounted."""
    import satisfiability_cases as K
    V, n, w, sub = c.num_vars, c.n, c.lookup_width, c.lookup_reps - 1
    full = np.array(c.variables, dtype=np.uint64)
    old = K.table_row_of(c, full, n - 1, sub)
    same = np.flatnonzero((c.tables[w] == c.tables[w, old]) & (c.tables[w - 1] != c.tables[w - 1, old]))
    for j in range(w):
        full[K.lookup_cell(c, sub, j), n - 1] = c.tables[j, int(same[0])]
    assert K.lookup_cell(c, sub, w - 1) == V - 1 and full[V - 1, n - 1] != c.variables[V - 1, n - 1]
    return full
