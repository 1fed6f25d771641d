"""-m gpu: proofs from a WitnessVec's values (bj_prove_values, bj_prove_values_async, bj_setup_set_witness_placement) and the kernel
behind them (witness_gather_kernel, csrc/witness_values.hip, through its door bj_witness_gather).  Everything is integer work and
every comparison is exact: the kernel against numpy's gather, a values proof against bj_prove on the columns numpy materialises
from the same placement and values, byte for byte (bj_prove's proofs are pinned against the oracle prover elsewhere).

The SHA-256 circuit's tables alone take 12320 rows, so its smallest trace has 2^14 rows: the whole-proof cases run at 2^14 and
2^16 rows (the smaller stands where 2^12 would).  That circuit has no public inputs; the public-input case puts some on it, on
variables that sit in several cells and on a placeholder."""
import ctypes as C
import dataclasses
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import memcopy_format as M
from era_boojum_amd import proof_format
from era_boojum_amd import sha256_circuit as S
from era_boojum_amd import synthetic
from gpu_util import ctx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)
PAIRINGS = {"poseidon2": {}, "poseidon": dict(transcript="poseidon", tree_hasher="poseidon"), "blake2s": dict(transcript="blake2s")}
SMALL, LARGE = 14, 16
INVALID, UNSUPPORTED = "invalid", "unsupported"


# ---------------------------------------------------------------- the kernel door
def gather_ref(placement, values):
    """witness_set_from_witness_vec on u32 cells: (cells, bad); a placeholder and an index beyond the values give 0."""
    p = placement.astype(np.int64)
    ok = (p != NONE) & (p < len(values))
    out = np.zeros(p.shape, dtype=np.uint64)
    out[ok] = values[p[ok]]
    return out, bool(((p != NONE) & ~ok).any())


def run_gather(placement, values, cols, log_n, offset_cells=0):
    """The door on `placement` (u32, cols << log_n cells) starting `offset_cells` cells into both device arrays; the cells in front
    and 8 cells behind the output must come back untouched."""
    c = ctx()
    count = cols << log_n
    assert placement.dtype == np.uint32 and placement.size == count
    raw = np.zeros(2 * ((offset_cells + count + 1) // 2 + 1), dtype=np.uint32)      # whole u64 words
    raw[offset_cells:offset_cells + count] = placement.reshape(-1)
    d_place = c.upload(raw.view(np.uint64))
    d_vals = c.upload(values if len(values) else np.zeros(1, dtype=np.uint64))
    total = offset_cells + count + 8
    d_cells = c.upload(np.full(total, SENTINEL, dtype=np.uint64))
    try:
        bad = c.witness_gather(d_place + 4 * offset_cells, cols, log_n, d_vals, len(values), d_cells + 8 * offset_cells)
        got = c.d2h(d_cells, (total,))
    finally:
        for d in (d_place, d_vals, d_cells):
            c.free(d)
    assert np.all(got[:offset_cells] == SENTINEL) and np.all(got[offset_cells + count:] == SENTINEL), "wrote outside its cells"
    return got[offset_cells:offset_cells + count], bad


def random_placement(rng, count, n_values, placeholders=0.1):
    p = rng.integers(0, n_values, size=count, dtype=np.int64).astype(np.uint32)
    p[rng.random(count) < placeholders] = NONE
    return p


def check_gather(placement, values, cols, log_n, offset_cells=0, expect_bad=False):
    want, bad = gather_ref(placement, values)
    assert bad == expect_bad
    got, got_bad = run_gather(placement, values, cols, log_n, offset_cells)
    assert np.array_equal(got, want)
    assert got_bad == expect_bad


@pytest.mark.parametrize("cols,log_n,offset", [
    (3, 1, 1),      # n = 2, 3 columns, the bases 4 and 8 bytes off a 16-byte boundary: scalar tail only
    (3, 1, 2),      # the placement 8 bytes off, the cells aligned: still no vector body
    (1, 10, 0), (93, 10, 0),
    (5, 0, 0), (6, 0, 0), (7, 0, 0),      # a vector body of one quad and a tail of 1, 2, 3 cells
    (1021, 0, 0),                         # four blocks of quads and a tail of 1
])
def test_gather_equals_numpy(cols, log_n, offset):
    rng = np.random.default_rng(1000 * cols + log_n)
    values = rng.integers(0, 1 << 64, size=777, dtype=np.uint64)      # any u64: the gather moves words, it does not reduce them
    check_gather(random_placement(rng, cols << log_n, len(values)), values, cols, log_n, offset)


def test_gather_placeholder_column_single_value_and_last_index():
    rng = np.random.default_rng(7)
    n, values = 1 << 10, rng.integers(0, 1 << 64, size=500, dtype=np.uint64)
    p = random_placement(rng, 3 * n, len(values)).reshape(3, n)
    p[1] = NONE                                             # an all-placeholder column: no load, zeros
    check_gather(p.reshape(-1), values, 3, 10)
    one = np.array([0x0123456789ABCDEF], dtype=np.uint64)   # n_values = 1: every cell names index 0 or nothing
    check_gather(random_placement(rng, n + 3, 1, 0.5), one, n + 3, 0)
    check_gather(np.full(2 * n + 1, len(values) - 1, dtype=np.uint32), values, 2 * n + 1, 0)   # every cell names index n_values - 1
    check_gather(np.full(5, NONE, dtype=np.uint32), np.zeros(0, dtype=np.uint64), 5, 0)         # no values at all


@pytest.mark.parametrize("where", ["body", "tail"])
def test_gather_flags_an_index_at_n_values(where):
    rng = np.random.default_rng(11)
    count, values = (1 << 10) + 3, rng.integers(0, 1 << 64, size=300, dtype=np.uint64)
    p = random_placement(rng, count, len(values))
    check_gather(p, values, count, 0)                       # the same cells without the bad one: no flag
    at = 517 if where == "body" else count - 2
    p[at] = len(values)
    want, _ = gather_ref(p, values)
    assert want[at] == 0
    check_gather(p, values, count, 0, expect_bad=True)      # flag set, that cell 0, every other cell still right


def test_gather_takes_a_second_trip_of_its_grid():
    sweep = ctx().witness_gather_sweep_cells()              # from the launcher's grid on this device
    assert sweep and sweep % 4 == 0
    log_n = 16
    cols = 2 * sweep // (1 << log_n) + 1                    # more than two sweeps: some lanes go round twice, some three times
    assert (cols << log_n) > 2 * sweep
    rng = np.random.default_rng(13)
    values = rng.integers(0, 1 << 64, size=1 << 20, dtype=np.uint64)
    check_gather(random_placement(rng, cols << log_n, len(values)), values, cols, log_n)
    count = sweep + 3                                       # one sweep of quads, then a scalar tail
    check_gather(random_placement(rng, count, len(values)), values, count, 0)


# ---------------------------------------------------------------- whole proofs
@functools.lru_cache(maxsize=None)
def sha(log_n):
    c, info = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(log_n), seed=11), return_info=True)
    assert c.log_n == log_n
    total = sum(t.shape[0] for t in S.sha_tables())
    counters = np.ascontiguousarray(c.multiplicities[0, :total].astype(np.uint32))
    assert not c.multiplicities[0, total:].any()
    return c, info["var_ids"], np.ascontiguousarray(info["all_values"], dtype=np.uint64), counters


def materialise(var_ids, all_values):
    return np.where(var_ids >= 0, all_values[np.maximum(var_ids, 0)], 0).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _setup(log_n, pairing):
    c, var_ids, _, _ = sha(log_n)
    return E.ProverSetup.from_placement(ctx(), c, var_ids, 8, 16, 30, **PAIRINGS[pairing])


def setup(log_n, pairing="poseidon2"):
    return _setup(log_n, pairing)


def reference_proofs(log_n, pairing="poseidon2"):
    return _reference_proofs(log_n, pairing)


@functools.lru_cache(maxsize=None)
def _reference_proofs(log_n, pairing):
    """bj_prove on the columns numpy materialises: (multiplicities supplied, counted).  Computed once, never changed."""
    c, var_ids, values, _ = sha(log_n)
    cols = materialise(var_ids, values)
    assert np.array_equal(cols, c.variables)
    s = setup(log_n, pairing)
    return s.prove(variables=cols)[0], s.prove(variables=cols, count_multiplicities=True)[0]


@pytest.mark.parametrize("log_n,pairing", [(SMALL, "poseidon2"), (LARGE, "poseidon2"), (SMALL, "poseidon"), (SMALL, "blake2s")])
def test_values_proof_is_the_proof_of_the_materialised_columns(log_n, pairing):
    _, _, values, counters = sha(log_n)
    supplied, counted = reference_proofs(log_n, pairing)
    s = setup(log_n, pairing)
    assert np.array_equal(s.prove_values(values, counters)[0], supplied)
    assert s.last_workspace["overflow_slabs"] == 0
    assert np.array_equal(s.prove_values(values, None)[0], counted)


def test_lean_values_proof_has_the_same_bytes():
    _, _, values, counters = sha(SMALL)
    supplied, counted = reference_proofs(SMALL)
    s = setup(SMALL)
    with ctx().lean_proofs(True):
        lean = s.prove_values(values, counters)[0]
        lean_ws = s.last_workspace["high_water_bytes"]     # the arena itself never shrinks on a context: what the proof took does
        lean_counted = s.prove_values(values, None)[0]
    assert np.array_equal(lean, supplied) and np.array_equal(lean_counted, counted)
    s.prove_values(values, counters)
    assert lean_ws < s.last_workspace["high_water_bytes"]    # it was lean


def test_prove_from_dumps_without_a_hint_is_the_values_proof():
    c, var_ids, values, counters = sha(SMALL)
    s = setup(SMALL)
    wit = M.write_witness_vec([], values, counters)
    without = s.prove_from_dumps(wit, None)[0]
    assert np.array_equal(without, s.prove_values(values, counters)[0])
    assert np.array_equal(without, s.prove_from_dumps(wit, M.write_variables_hint(var_ids))[0])     # the path with a hint, as before
    assert np.array_equal(without, reference_proofs(SMALL)[0])


# ---------------------------------------------------------------- witness columns
@functools.lru_cache(maxsize=None)
def witness_case():
    """synthetic.witness_gates at 2^10 rows.  Variables: the identity over the flattened columns.  Witness columns: every distinct
    value once behind them, so equal cells share an index (repeats), and some of the zero cells are placeholders instead."""
    c = synthetic.sha_shaped_circuit(10, seed=5, table_bits=2, gates=synthetic.witness_gates(60, 4, 5), mix=(0.05, 0.3, 0.3, 0.2),
                                     num_witness_cols=5)
    V, n = c.variables.shape
    var_ids = np.arange(V * n, dtype=np.int64).reshape(V, n)
    uniq, inverse = np.unique(c.witness, return_inverse=True)
    wit_ids = (V * n + inverse.reshape(c.witness.shape)).astype(np.int64)
    rng = np.random.default_rng(3)
    wit_ids[(c.witness == 0) & (rng.random(c.witness.shape) < 0.5)] = -1
    values = np.concatenate([c.variables.reshape(-1), uniq]).astype(np.uint64)
    assert (wit_ids < 0).any() and len(uniq) < c.witness.size and np.array_equal(materialise(wit_ids, values), c.witness)
    return c, var_ids, wit_ids, values


def test_witness_columns_come_through_their_own_placement():
    c, var_ids, wit_ids, values = witness_case()
    total = int(np.flatnonzero(c.multiplicities[0])[-1]) + 1
    counters = np.ascontiguousarray(c.multiplicities[0, :total].astype(np.uint32))
    s = E.ProverSetup.from_placement(ctx(), c, var_ids, 8, 16, 30)
    try:
        before = s.device_bytes()
        with pytest.raises(E.BoojumHipError, match=INVALID + ".*5 non-copiable witness columns and no witness placement"):
            s.prove_values(values, counters)
        s.set_witness_placement(wit_ids)
        assert s.device_bytes() == before + 4 * wit_ids.size
        want = s.prove()[0]                                   # bj_prove on the numpy columns (the circuit's own)
        assert np.array_equal(s.prove_values(values, counters)[0], want)
        assert np.array_equal(s.prove_values(values, None)[0], s.prove(count_multiplicities=True)[0])
        s.set_witness_placement(wit_ids)                      # set again: replaced, not leaked
        assert s.device_bytes() == before + 4 * wit_ids.size
        assert np.array_equal(s.prove_values(values, counters)[0], want)
        pub = proof_format.parse(want, security_level=30)["public_inputs"]
        assert pub == [int(p[2]) for p in c.public_inputs] and len(pub) == 2
    finally:
        s.close()


# ---------------------------------------------------------------- async
@functools.lru_cache(maxsize=None)
def second_witness():
    """Another satisfied witness for the same setup: the SHA circuit's placement depends on the message length alone, so another
    message of that length gives other all_values and counters under the same placement."""
    _, var_ids, values, counters = sha(SMALL)
    c2, info2 = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(SMALL), seed=12), return_info=True)
    assert np.array_equal(info2["var_ids"], var_ids), "the placement depends on the message"
    values2 = np.ascontiguousarray(info2["all_values"], dtype=np.uint64)
    assert not np.array_equal(values2, values)
    return c2, values2, np.ascontiguousarray(c2.multiplicities[0, :len(counters)].astype(np.uint32))


def test_async_alternates_two_all_values_between_plain_async_proofs():
    _, _, values, counters = sha(SMALL)
    c2, values2, counters2 = second_witness()
    s = setup(SMALL)
    serial = [s.prove_values(values, counters)[0], s.prove_values(values2, counters2)[0]]
    assert np.array_equal(serial[0], reference_proofs(SMALL)[0]) and not np.array_equal(serial[0], serial[1])
    assert np.array_equal(serial[1], s.prove(variables=c2.variables, multiplicities=c2.multiplicities)[0])
    w = [(values, counters), (values2, counters2)]
    columns = np.ascontiguousarray(c2.variables)
    tickets, want, got = [], [], []
    for k in range(6):                                        # t[k] = async; wait(t[k-1])
        tickets.append(s.prove_values_async(*w[k % 2]))
        want.append(serial[k % 2])
        if len(tickets) == 2:
            got.append(s.wait(tickets.pop(0))[0])
        if k in (1, 4):                                       # plain bj_prove_async submissions on the same context, in between
            tickets.append(s.prove_async(variables=columns, multiplicities=c2.multiplicities))
            want.append(serial[1])
            got.append(s.wait(tickets.pop(0))[0])
    got += [s.wait(t)[0] for t in tickets]
    assert len(got) == len(want) == 8
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), k


# ---------------------------------------------------------------- admission (fresh child processes)
@pytest.mark.parametrize("case", ["values_lane_lean", "values_refuse"])
def test_values_admission(case):
    env = {k: v for k, v in os.environ.items() if k not in ("BJ_HBM_BUDGET_BYTES", "BJ_PROOF_LEAN", "BJ_ASYNC_MODE")}
    env["BJ_ASYNC_DEBUG"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "prove_values_admission_worker.py"), case], env=env, capture_output=True, text=True,
                       timeout=180)
    print(r.stdout[-6000:])
    print(r.stderr[-6000:])
    assert r.returncode == 0 and "case %s holds" % case in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------- refusals
def test_refusals_carry_a_status_and_a_message():
    c, var_ids, values, counters = sha(SMALL)
    n = 1 << c.log_n
    s = setup(SMALL)
    good = s.prove_values(values, counters)[0]
    host = E.ProverSetup(ctx(), c, 8, 16, 30)                 # from host sigmas: no placement
    try:
        for call in (host.prove_values, host.prove_values_async):
            with pytest.raises(E.BoojumHipError, match=INVALID + ".*holds no variable placement"):
                call(values, counters)
    finally:
        host.close()
    short = np.ascontiguousarray(values[:int(var_ids.max())])  # one value short of what the placement names
    with pytest.raises(E.BoojumHipError, match=INVALID + ".*a cell names a variable beyond all_values"):
        s.prove_values(short, counters)
    assert np.array_equal(s.prove_values(values, counters)[0], good)      # the context is none the worse
    t = s.prove_values_async(short, counters)                 # on a lane the refusal is the proof's: it comes back from the wait
    with pytest.raises(E.BoojumHipError, match=INVALID + ".*a cell names a variable beyond all_values"):
        s.wait(t)
    assert np.array_equal(s.wait(s.prove_values_async(values, counters))[0], good)
    too_many = np.zeros(n + 1, dtype=np.uint32)
    for call in (s.prove_values, s.prove_values_async):
        with pytest.raises(E.BoojumHipError, match=INVALID + ".*%d multiplicities for %d rows" % (n + 1, n)):
            call(values, too_many)
    lib, h = ctx()._lib, C.c_void_p()
    m = counters.ctypes.data_as(C.c_void_p)
    for fn in (lib.bj_prove_values, lib.bj_prove_values_async):
        rc = fn(ctx()._h, s._h, None, len(values), m, len(counters), C.byref(h))
        assert rc < 0 and not h.value
        assert b"invalid" in lib.bj_status_string(rc) and b"null h_values with n_values" in lib.bj_last_error(ctx()._h)
        assert rc == lib.bj_prove_values(ctx()._h, None, None, 0, None, 0, C.byref(h))      # the status of any null argument
    assert np.array_equal(s.prove_values(values, counters)[0], good)


def test_a_sharded_setup_is_unsupported():
    """Both ranks of a two-way sharded setup (threads of this process, binding.ThreadGroup)."""
    c = synthetic.sha_shaped_circuit(10, seed=21, table_bits=2)
    values = np.ascontiguousarray(c.variables.reshape(-1))
    group, out, errors = E.ThreadGroup(2), [None, None], []

    def rank(r):
        try:
            cx = E.Context(0)
            s = E.ProverSetup(cx, c, 8, 16, 30, comm=group.comm(cx, r))
            msgs = []
            for call in (s.prove_values, s.prove_values_async):
                try:
                    call(values, None)
                    msgs.append("no error")
                except E.BoojumHipError as e:
                    msgs.append(str(e))
            out[r] = msgs
            s.close()
            cx.close()
        except Exception as e:      # noqa: BLE001 - reported by the main thread
            errors.append(e)
            try:
                group._barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for msgs in out:
        assert len(msgs) == 2 and all(UNSUPPORTED in m and "single-device setups only" in m for m in msgs), msgs


# ---------------------------------------------------------------- public inputs
def test_public_inputs_are_read_through_the_placement():
    c, var_ids, values, counters = sha(SMALL)
    uses = np.bincount(var_ids[var_ids >= 0])
    shared = np.flatnonzero(uses >= 3)[:3]                    # variables placed in several cells
    assert len(shared) == 3
    locs = []
    for k, v in enumerate(shared):
        cells = np.argwhere(var_ids == v)
        col, row = cells[k % len(cells)]                      # not always the first of its cells
        locs.append((int(col), int(row)))
    hole = np.argwhere(var_ids < 0)[5]
    locs.append((int(hole[0]), int(hole[1])))                 # a public input on a placeholder cell: value 0
    cols = materialise(var_ids, values)
    pubs = [(col, row, int(cols[col, row])) for col, row in locs]
    c2 = dataclasses.replace(c, public_inputs=pubs)
    s = E.ProverSetup.from_placement(ctx(), c2, var_ids, 8, 16, 30)
    try:
        proof = s.prove_values(values, counters)[0]
        words = proof_format.parse(proof, security_level=30)["public_inputs"]
        assert words == [int(values[var_ids[col, row]]) for col, row in locs[:3]] + [0]
        assert words == [p[2] for p in pubs] and len(set(words[:3])) > 1
        assert np.array_equal(proof, s.prove(variables=cols)[0])
        assert not np.array_equal(proof, reference_proofs(SMALL)[0])      # the public inputs are in the transcript
        wit = M.write_witness_vec(locs, values, counters)
        assert np.array_equal(s.prove_from_dumps(wit, None)[0], proof)
    finally:
        s.close()
