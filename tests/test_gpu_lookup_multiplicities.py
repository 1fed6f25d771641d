"""-m gpu: the multiplicity column counted on the device (csrc/lookup_multiplicities.hip) — bj_lookup_multiplicities on raw
columns, bj_setup_lookup_multiplicities on a setup, and bj_prove / bj_prove_dev / bj_prove_async without a column.  The expected
column is counted here with numpy: equal table rows are grouped and the count goes to the first row of the group."""
import ctypes as C
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import field_np as F
from era_boojum_amd import proof_format
from era_boojum_amd import synthetic as S
from gpu_util import ctx
from oracle import verifier as OV

import satisfiability_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DISTINCT = ["sha10", "sha13", "tidvar13", "golden10", "spec10"]   # pairwise distinct real table rows, no lookup of the padding class
FRI, CAP, SEC = 8, 16, 30


@functools.lru_cache(maxsize=None)
def setup(name, relooked=0):
    c = K.relooked(name, relooked) if relooked else K.circuit(name)
    return E.ProverSetup(ctx(), c, FRI, CAP, SEC)


def raw_columns(c, full=None):
    """(lookup columns [reps * cps][n], table id column [n] or None, tables [w + 1][n]) as bj_lookup_multiplicities takes them."""
    full = K.full_witness(c) if full is None else full
    lo = c.num_gp_vars
    lvars = np.array(full[lo:lo + c.lookup_reps * c.lookup_cols_per_sub], dtype=np.uint64)
    tid = None if c.table_id_as_variable else np.array(c.constants[c.table_id_col], dtype=np.uint64)
    return lvars, tid, np.array(c.tables, dtype=np.uint64)


def numpy_count(lvars, tid, tables, reps, w):
    """The column by definition: (multiplicities [n], looked-up tuples that are in no table row)."""
    n = tables.shape[1]
    cps = lvars.shape[0] // reps
    tuples = []
    for sub in range(reps):
        cols = [lvars[sub * cps + j] for j in range(w)] + [lvars[sub * cps + w] if tid is None else tid]
        tuples.append(np.stack(cols, axis=1))
    rows = F.canon(np.ascontiguousarray(np.concatenate([tables.T] + tuples, axis=0)))
    _, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    classes = int(inv.max()) + 1
    first = np.full(classes, n, dtype=np.int64)
    np.minimum.at(first, inv[:n], np.arange(n))                    # the first table row of every class; n: no table row holds it
    counts = np.bincount(inv[n:], minlength=classes)
    out = np.zeros(n, dtype=np.uint64)
    held = first < n
    out[first[held]] = counts[held].astype(np.uint64)
    return out, int(counts[~held].sum())


def expected(c, full=None):
    out, misses = numpy_count(*raw_columns(c, full), c.lookup_reps, c.lookup_width)
    assert misses == 0
    return out.reshape(1, c.n)


def operator_count(lvars, tid, tables, reps, w, var_pad=3, table_pad=5):
    """bj_lookup_multiplicities on columns laid out with strides n + var_pad / n + table_pad (odd: no column is aligned)."""
    cx, n = ctx(), tables.shape[1]

    def strided(a, pad):
        buf = np.full((a.shape[0], n + pad), 0xDEADBEEF, dtype=np.uint64)
        buf[:, :n] = a
        return buf
    d_v, d_t, d_out = cx.upload(strided(lvars, var_pad)), cx.upload(strided(tables, table_pad)), cx.malloc(8 * n)
    d_id = cx.upload(tid) if tid is not None else None
    try:
        cx.lookup_multiplicities(d_v, n + var_pad, d_id, d_t, n + table_pad, reps, w, n.bit_length() - 1, d_out)
        return cx.d2h(d_out, (n,))
    finally:
        for p in (d_v, d_t, d_out, d_id):
            if p is not None:
                cx.free(p)


def verifies(s, proof):
    return OV.verify(OV.VerificationKey(s.circuit, s.cap(), FRI, CAP), proof_format.parse(proof, security_level=SEC))


@pytest.mark.parametrize("name", DISTINCT)
def test_counted_equals_host(name):
    s = setup(name)
    c = s.circuit
    T = c.total_tables_len
    real = F.canon(np.ascontiguousarray(c.tables[:, :T].T))
    assert len(np.unique(real, axis=0)) == T                           # the precondition: distinct real rows,
    assert not np.any(c.multiplicities[0, T:]) and int(c.multiplicities.sum()) == c.n * c.lookup_reps   # nothing on the padding class
    assert np.array_equal(expected(c), c.multiplicities)
    assert np.array_equal(s.count_multiplicities(K.full_witness(c)), c.multiplicities)
    got = operator_count(*raw_columns(c), c.lookup_reps, c.lookup_width)
    assert np.array_equal(got, c.multiplicities[0])


@pytest.mark.parametrize("name", ["sha10", "tidvar13"])
def test_noncanonical_cells(name):
    s = setup(name)
    c = s.circuit
    nc = K.noncanonical(K.full_witness(c))
    assert np.any(nc != K.full_witness(c))
    assert np.array_equal(s.count_multiplicities(nc), c.multiplicities)
    lvars, tid, tables = raw_columns(c)
    got = operator_count(K.noncanonical(lvars), None if tid is None else K.noncanonical(tid), K.noncanonical(tables), c.lookup_reps,
                         c.lookup_width)
    assert np.array_equal(got, c.multiplicities[0])


@pytest.mark.parametrize("name,rows", [("sha10", 16), ("sha10", 1021), ("tidvar13", 16)])
def test_equal_table_rows_are_one_class(name, rows):
    s = setup(name, rows)
    c = s.circuit
    host = c.multiplicities
    assert host[0, 0] and host[0, rows - 1]                            # the host column splits the class over its two rows
    if (name, rows) == ("sha10", 16):
        assert (int(host[0, 0]), int(host[0, 15])) == (513, 547)
    counted = s.count_multiplicities(K.full_witness(c))
    want = host.copy()
    want[0, 0], want[0, rows - 1] = host[0, 0] + host[0, rows - 1], 0
    assert np.array_equal(counted, want) and np.array_equal(counted, expected(c))
    assert s.check_satisfied(K.full_witness(c), counted).kind == E.binding.SAT


def test_padding_class():
    s = setup("tidvar13")
    c = s.circuit
    row, sub, T = 4321, 2, c.total_tables_len
    full = K.full_witness(c)
    old = K.table_row_of(c, full, row, sub)
    for j in range(c.lookup_width + 1):
        full[K.lookup_cell(c, sub, j), row] = 0
    counted = s.count_multiplicities(full)
    assert np.array_equal(counted, expected(c, full))
    assert counted[0, T] == 1 and not np.any(counted[0, T + 1:])
    assert counted[0, old] == c.multiplicities[0, old] - 1
    want = c.multiplicities.copy()
    want[0, old] -= 1
    want[0, T] = 1
    assert np.array_equal(counted, want)


def _tidvar_shape(pick):
    """Raw columns of tidvar13's shape in which row i of every sub-argument looks table row pick[i] up."""
    c = K.circuit("tidvar13")
    tables = np.array(c.tables, dtype=np.uint64)
    lvars = np.empty((c.lookup_reps * c.lookup_cols_per_sub, c.n), dtype=np.uint64)
    for sub in range(c.lookup_reps):
        for j in range(c.lookup_width + 1):
            lvars[sub * c.lookup_cols_per_sub + j] = tables[j][pick]
    return c, lvars, tables


@pytest.mark.parametrize("shape", ["one_class", "64_distinct", "alternating"])
def test_wave_aggregation_shapes(shape):
    c0 = K.circuit("tidvar13")
    n, T = c0.n, c0.total_tables_len
    assert T >= 64
    i = np.arange(n)
    pick = {"one_class": np.full(n, 5), "64_distinct": (i * 37 + 11) % 64, "alternating": np.where(i % 2 == 0, 3, T - 1)}[shape]
    c, lvars, tables = _tidvar_shape(pick)
    want, misses = numpy_count(lvars, None, tables, c.lookup_reps, c.lookup_width)
    assert misses == 0 and int(want.sum()) == n * c.lookup_reps
    if shape == "one_class":
        assert want[5] == n * c.lookup_reps
    if shape == "64_distinct":
        assert np.count_nonzero(want) == 64                            # every wave of 64 consecutive rows holds 64 classes
    got = operator_count(lvars, None, tables, c.lookup_reps, c.lookup_width)
    assert np.array_equal(got, want)


MISS = r"invalid.*row %d by sub-argument %d is in no table row \(%d such lookups\)"


@pytest.mark.parametrize("name", ["sha10", "tidvar13"])
def test_a_miss_is_named(name):
    s = setup(name)
    c = s.circuit
    n, last = c.n, c.lookup_reps - 1
    d_out = ctx().malloc(8 * n)
    try:
        for row, sub in ((0, 0), (n - 1, last)):
            full = K.plant_lookup_miss(c, row, sub)
            assert numpy_count(*raw_columns(c, full), c.lookup_reps, c.lookup_width)[1] == 1
            d_v = ctx().upload(full)
            try:
                assert s._lib.bj_setup_lookup_multiplicities(ctx()._h, s._h, d_v, d_out) == -1
                with pytest.raises(E.BoojumHipError, match=MISS % (row, sub, 1)):
                    s.count_multiplicities_dev(d_v, d_out)
            finally:
                ctx().free(d_v)
        both = K.plant_lookup_miss(c, n - 1, last, K.plant_lookup_miss(c, 0, 0))
        with pytest.raises(E.BoojumHipError, match=MISS % (0, 0, 2)):
            s.count_multiplicities(both)
        with pytest.raises(E.BoojumHipError, match=MISS % (0, 0, 2)):
            operator_count(*raw_columns(c, both), c.lookup_reps, c.lookup_width)
        d_v = ctx().upload(both)
        try:
            with pytest.raises(E.BoojumHipError, match=MISS % (0, 0, 2)):      # refused before any proof work: no proof comes back
                s.prove_dev(d_v, None, count_multiplicities=True)
        finally:
            ctx().free(d_v)
        with pytest.raises(E.BoojumHipError, match=MISS % (0, 0, 2)):
            s.prove(both, count_multiplicities=True)
    finally:
        ctx().free(d_out)
    s.prove()                                                          # the context proves on


@pytest.mark.parametrize("name", ["sha10", "tidvar13", "golden10"])
def test_proofs_without_a_column(name):
    s = setup(name)
    c = s.circuit
    full = K.full_witness(c)
    d_v, d_m = ctx().upload(full), ctx().upload(c.multiplicities)
    try:
        before, _ = s.prove_dev(d_v, d_m)
        assert s.last_workspace["overflow_slabs"] == 0
        counted, _ = s.prove_dev(d_v, None, count_multiplicities=True)
        assert s.last_workspace["overflow_slabs"] == 0
        after, _ = s.prove_dev(d_v, d_m)                               # a supplied column after a counted one: as before it
        assert np.array_equal(counted, before) and np.array_equal(after, before)
        assert np.array_equal(ctx().d2h(d_v, full.shape), full) and np.array_equal(ctx().d2h(d_m, (1, c.n)), c.multiplicities)
    finally:
        ctx().free(d_v)
        ctx().free(d_m)
    assert verifies(s, counted)
    host, _ = s.prove(full, count_multiplicities=True)                 # bj_prove: counted once the last column group has landed
    assert s.last_workspace["overflow_slabs"] == 0
    assert np.array_equal(host, before)
    tickets = [s.prove_async(full, count_multiplicities=True) for _ in range(2)]   # two in flight, each lane counts in its own scratch
    for t in tickets:
        proof, _ = s.wait(t)
        assert s.last_workspace["overflow_slabs"] == 0
        assert np.array_equal(proof, before)


def test_proof_of_a_circuit_with_equal_table_rows():
    s = setup("sha10", 16)
    c = s.circuit
    full = K.full_witness(c)
    d_v = ctx().upload(full)
    try:
        counted, _ = s.prove_dev(d_v, None, count_multiplicities=True)
        assert s.last_workspace["overflow_slabs"] == 0
    finally:
        ctx().free(d_v)
    host, _ = s.prove()
    assert verifies(s, counted) and verifies(s, host)
    assert not np.array_equal(counted, host)                           # another multiplicity column is another witness oracle


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_proof_without_a_column(tmp_path):
    """Two ranks over gloo on this GPU, no column on either: each counts on its replicated columns; the single-GPU bytes."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "lookup_multiplicities_worker.py"), str(tmp_path), "sha10",
           str(FRI), str(CAP), str(SEC)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    single, _ = setup("sha10").prove()
    for rank in range(2):
        assert np.array_equal(np.load(os.path.join(str(tmp_path), "proof_%d.npy" % rank)), single), "rank %d" % rank
        assert np.array_equal(np.load(os.path.join(str(tmp_path), "column_%d.npy" % rank)), K.circuit("sha10").multiplicities)


def test_argument_errors():
    s = setup("sha10")
    c = s.circuit
    lib, h, n = s._lib, ctx()._h, c.n
    lvars, tid, tables = raw_columns(c)
    d_v, d_out, d_l, d_id, d_t = ctx().upload(c.variables), ctx().malloc(8 * n), ctx().upload(lvars), ctx().upload(tid), ctx().upload(tables)
    plain = E.ProverSetup(ctx(), S.sha_shaped_circuit(8, seed=2, table_bits=2, lookup_reps=0), FRI, CAP, SEC)   # a circuit without lookups
    try:
        assert lib.bj_setup_lookup_multiplicities(h, s._h, None, d_out) == -1
        assert lib.bj_setup_lookup_multiplicities(h, s._h, d_v, None) == -1
        assert lib.bj_setup_lookup_multiplicities(h, None, d_v, d_out) == -1
        args = (c.lookup_reps, c.lookup_width, c.log_n)
        assert lib.bj_lookup_multiplicities(h, None, n, d_id, d_t, n, *args, d_out) == -1
        assert lib.bj_lookup_multiplicities(h, d_l, n, d_id, None, n, *args, d_out) == -1
        assert lib.bj_lookup_multiplicities(h, d_l, n, d_id, d_t, n, *args, None) == -1
        assert lib.bj_lookup_multiplicities(h, d_l, n, d_id, d_t, n, 0, c.lookup_width, c.log_n, d_out) == -1
        assert b"bj_lookup_multiplicities" in lib.bj_last_error(h)
        assert lib.bj_lookup_multiplicities(h, d_l, n - 1, d_id, d_t, n, *args, d_out) == -1
        assert lib.bj_lookup_multiplicities(h, d_l, n, d_id, d_t, n, c.lookup_reps, 16, c.log_n, d_out) == -5      # BJ_ERR_UNSUPPORTED
        assert lib.bj_lookup_multiplicities(h, d_l, 1 << 31, d_id, d_t, 1 << 31, c.lookup_reps, c.lookup_width, 31, d_out) == -5
        assert lib.bj_lookup_multiplicities(h, d_l, n, d_id, d_t, n, *args, d_out) == 0
        assert np.array_equal(ctx().d2h(d_out, (1, n)), c.multiplicities)
        assert lib.bj_setup_lookup_multiplicities(h, plain._h, d_v, d_out) == -1
        assert b"no lookups" in lib.bj_last_error(h)
    finally:
        for p in (d_v, d_out, d_l, d_id, d_t):
            ctx().free(p)
        plain.close()
