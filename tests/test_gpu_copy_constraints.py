"""-m gpu: bj_sigma_cells and bj_check_copy_constraints (csrc/copy_check.hip).  Everything is integer work and every comparison is
exact.  Expected values come from numpy (tests/copy_constraint_cases.py): identities k_c * omega^row from field_np, sigma from
sha256_circuit.sigma_from_placement on random sparse placements, the cell of each sigma word from np.searchsorted over the sorted
identities, the report from v != v[perm] and a bincount of the targets."""
import dataclasses
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding
from era_boojum_amd import sha256_circuit as SHA
from era_boojum_amd import synthetic
from gpu_util import ctx

import copy_constraint_cases as CC
import satisfiability_cases as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO_CELL = CC.NO_CELL
SENTINEL64, SENTINEL32 = np.uint64(0xDEADBEEFDEADBEEF), np.uint32(0xDEADBEEF)
SIZES = [(1, 2), (5, 1), (5, 3), (10, 92), (16, 3)]


def device_cells(sig, log_n, ks, pad_in=8, pad_out=24):
    """bj_sigma_cells with padded strides on both sides -> (cells [V][n] u32, first_invalid, num_invalid)."""
    V, n = sig.shape
    c = ctx()
    src = np.full((V, n + pad_in), SENTINEL64, dtype=np.uint64)
    src[:, :n] = sig
    dst = np.full((V, n + pad_out), SENTINEL32, dtype=np.uint32)      # an even number of u32 per column: uploaded as u64 words
    d_in, d_out = c.upload(src), c.upload(dst.reshape(-1).view(np.uint64))
    try:
        first, count = c.sigma_cells(d_in, V, log_n, ks, d_out, sig_stride=n + pad_in, cell_stride=n + pad_out)
        got = c.d2h(d_out, (dst.size // 2,)).view(np.uint32).reshape(dst.shape)
        assert np.array_equal(c.d2h(d_in, src.shape), src), "the input was written"
    finally:
        c.free(d_in)
        c.free(d_out)
    assert np.all(got[:, n:] == SENTINEL32), "wrote between the columns"
    return got[:, :n], first, count


@functools.lru_cache(maxsize=None)
def sigma_case(log_n, V):
    ks = synthetic.non_residues(V, 1 << log_n)
    sig = CC.sigma_from_placement(CC.sparse_placement(log_n, V, seed=100 * log_n + V), log_n, ks)
    want = CC.expected_cells(sig, log_n, ks)
    assert not np.any(want == NO_CELL) and np.array_equal(np.sort(want.reshape(-1)), np.arange(V << log_n))
    assert not np.array_equal(want.reshape(-1), np.arange(V << log_n)), "the placement links nothing"
    sig.setflags(write=False)
    want.setflags(write=False)
    return ks, sig, want


@pytest.mark.parametrize("log_n,V", SIZES)
def test_operator_inverts_sigma(log_n, V):
    ks, sig, want = sigma_case(log_n, V)
    for words in (sig, K.noncanonical(sig)):               # canonical, then p added to every word below 2^32 - 1
        got, first, count = device_cells(words, log_n, ks)
        assert np.array_equal(got, want)
        assert (first, count) == (None, 0)
    assert np.any(K.noncanonical(sig) != sig)


@pytest.mark.parametrize("log_n,V", [(5, 3), (10, 92)])
def test_operator_marks_words_in_no_coset(log_n, V):
    ks, sig, _ = sigma_case(log_n, V)
    n = 1 << log_n
    outside = synthetic.non_residues(V + 1, n)[V]                       # the next non-residue: a coset of its own
    om = CC.identities(1, log_n, [1])[0]
    word = lambda r: int(outside) * int(om[r]) % E.P                    # noqa: E731
    bad = np.array(sig)
    places = {(0, 0): 0, (V // 2, n - 1): word(n - 1), (V - 1, 0): word(0), (V - 1, n // 2): 0, (V - 1, n - 1): word(3)}
    for (col, row), w in places.items():
        bad[col, row] = w
    want = CC.expected_cells(bad, log_n, ks)
    assert {(int(c), int(r)) for c, r in zip(*np.nonzero(want == NO_CELL))} == set(places)
    got, first, count = device_cells(bad, log_n, ks)
    assert np.array_equal(got, want)
    assert (first, count) == (0, len(places))                           # key of (column 0, row 0)
    bad[0, 0] = sig[0, 0]
    got, first, count = device_cells(bad, log_n, ks)
    assert np.array_equal(got, CC.expected_cells(bad, log_n, ks))
    assert (first, count) == (0 * V + V - 1, len(places) - 1)           # now (column V - 1, row 0)


def test_operator_refusals_carry_a_status_and_a_message():
    d = ctx().malloc(64)
    try:
        for V, log_n, ks, match in ((1, 31, [1], "unsupported.*log_n 31 > 30"),
                                    (4, 30, synthetic.non_residues(4, 1 << 30), r"unsupported.*num_vars \* n < 2\^32"),
                                    (3, 3, [1, 7, 7], "invalid.*non-residues 1 and 2 name the same coset")):
            with pytest.raises(E.BoojumHipError, match=match):
                ctx().sigma_cells(d, V, log_n, ks, d)
            assert len(ctx()._lib.bj_last_error(ctx()._h)) > 0
    finally:
        ctx().free(d)


# ---- the check on setups ----

def fields(r):
    return (r.kind, r.column, r.row, r.partner_column, r.partner_row, r.value, r.partner_value, r.variable, r.failures)


@functools.lru_cache(maxsize=None)
def free_setups():
    """The crafted circuit as a setup from host sigmas and as a setup from the placement."""
    c, var_ids = CC.free_circuit()
    return E.ProverSetup(ctx(), c, 8, 16, 30), E.ProverSetup.from_placement(ctx(), c, var_ids, 8, 16, 30)


@functools.lru_cache(maxsize=None)
def sha16():
    c, info = SHA.sha256_circuit(SHA.bench_message(SHA.message_len_for_log_n(16), seed=11), return_info=True)
    assert c.log_n == 16
    return c, E.ProverSetup(ctx(), c, 8, 16, 30)


def honest(s, c):
    """COPY_OK with all counts 0, and the proof after the check is the proof before it."""
    d_v, d_m = ctx().upload(c.variables), ctx().upload(c.multiplicities)
    try:
        before, _ = s.prove_dev(d_v, d_m)
        r = s.check_copy_constraints(d_v)
        after, _ = s.prove_dev(d_v, d_m)
        assert np.array_equal(ctx().d2h(d_v, c.variables.shape), c.variables)
    finally:
        ctx().free(d_v)
        ctx().free(d_m)
    assert fields(r) == (binding.COPY_OK, 0, 0, 0, 0, 0, 0, NO_CELL, (0, 0, 0, 0)) and bool(r)
    assert np.array_equal(before, after)
    assert CC.check(c.sigmas, c.variables, c.log_n, c.non_residues).kind == 0


def test_honest_witness_synthetic_2p10():
    c, _ = CC.free_circuit()
    for s in free_setups():
        honest(s, c)


def test_honest_witness_sha256_2p16():
    c, s = sha16()
    honest(s, c)


@pytest.mark.parametrize("which", ["first", "public", "random", "last"])
def test_value_mutations(which):
    """One changed cell in a cycle: every gate still holds (bj_check_satisfied: BJ_SAT), the prover refuses without naming
    anything, and the new check names the cell, its partner, both values and the variable, as numpy's v != v[perm] does."""
    c, var_ids = CC.free_circuit()
    V, n = c.num_vars, c.n
    plain, placed = free_setups()
    perm = CC.expected_cells(c.sigmas, c.log_n, c.non_residues).reshape(-1)
    public_values = [p[2] for p in c.public_inputs]
    if which == "last":
        col, row = V - 1, n - 1
        full = CC.moved_last_tuple(c)
    else:
        if which == "random":
            linked = np.flatnonzero(perm[:c.num_gp_vars * n] != np.arange(c.num_gp_vars * n))
            cell = int(linked[np.random.default_rng(5).integers(len(linked))])
            col, row = cell // n, cell % n
        else:
            col, row = CC.FIRST if which == "first" else CC.PUBLIC
        full = CC.changed(c.variables, col, row)
        if which == "public":                              # the public value follows the cell: only the copy constraint breaks
            public_values[0] = int(full[col, row])
    assert perm[col * n + row] != col * n + row, "the changed cell is in no cycle"
    want = CC.check(c.sigmas, full, c.log_n, c.non_residues, var_ids)
    assert want.kind == binding.COPY_VALUE_MISMATCH and want.failures[3] >= 2 and want.variable != NO_CELL
    if which == "first":
        assert (want.column, want.row) == CC.FIRST
    d_v = ctx().upload(full)
    d_m = ctx().malloc(8 * n)
    try:
        placed.count_multiplicities_dev(d_v, d_m)
        got = placed.check_copy_constraints(d_v)
        assert fields(got) == want.fields() and not got
        without_placement = plain.check_copy_constraints(d_v)
        assert fields(without_placement) == dataclasses.replace(want, variable=NO_CELL).fields()
        assert placed.check_satisfied_dev(d_v, d_m).kind == binding.SAT
        with pytest.raises(E.BoojumHipError, match="not satisfied"):
            placed.prove_dev(d_v, d_m, public_values)
    finally:
        ctx().free(d_v)
        ctx().free(d_m)


def test_sigma_that_is_no_permutation_and_sigma_with_a_word_in_no_coset():
    c, _ = CC.free_circuit()
    V, n = c.num_vars, c.n
    sig = np.array(c.sigmas)
    sig[5, 700], sig[30, 2] = sig[2, 9], sig[2, 9]               # three entries name one target, none of them the smallest key
    sig[V - 1, n - 1] = sig[0, 0]
    want = CC.check(sig, c.variables, c.log_n, c.non_residues)
    assert want.kind == binding.COPY_SIGMA_NOT_PERMUTATION and want.failures[2] == 3 and (want.column, want.row) == (0, 0)
    d_v = ctx().upload(c.variables)
    try:
        s = E.ProverSetup(ctx(), dataclasses.replace(c, sigmas=sig), 8, 16, 30)
        try:
            assert fields(s.check_copy_constraints(d_v)) == want.fields()
        finally:
            s.close()
        sig[V - 1, n - 1] = c.sigmas[V - 1, n - 1]              # without the pair at key 0 the named source is (30, 2)
        want = CC.check(sig, c.variables, c.log_n, c.non_residues)
        assert (want.kind, want.column, want.row, want.failures[2]) == (2, 30, 2, 2)
        s = E.ProverSetup(ctx(), dataclasses.replace(c, sigmas=sig), 8, 16, 30)
        try:
            assert fields(s.check_copy_constraints(d_v)) == want.fields()
        finally:
            s.close()
        sig[60, 1023] = 0                                        # kind 1 comes first, the other counts are still filled
        sig[1, 4] = int(synthetic.non_residues(V + 1, n)[V]) * int(CC.identities(1, c.log_n, [1])[0][17]) % E.P
        want = CC.check(sig, c.variables, c.log_n, c.non_residues)
        assert (want.kind, want.column, want.row, want.failures[1], want.failures[2]) == (1, 1, 4, 2, 2)
        s = E.ProverSetup(ctx(), dataclasses.replace(c, sigmas=sig), 8, 16, 30)
        try:
            assert fields(s.check_copy_constraints(d_v)) == want.fields()
        finally:
            s.close()
    finally:
        ctx().free(d_v)


def test_argument_errors():
    import ctypes as C
    plain, _ = free_setups()
    lib, h = plain._lib, ctx()._h
    d_v = ctx().upload(plain.circuit.variables)
    rep = binding._CopyReport()
    try:
        assert lib.bj_check_copy_constraints(h, plain._h, d_v, None) == -1
        assert lib.bj_check_copy_constraints(h, plain._h, None, C.byref(rep)) == -1
        assert lib.bj_check_copy_constraints(h, None, d_v, C.byref(rep)) == -1
        assert b"null argument" in lib.bj_last_error(h)
        assert lib.bj_check_copy_constraints(h, plain._h, d_v, C.byref(rep)) == 0 and rep.kind == 0
    finally:
        ctx().free(d_v)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_setup_gives_the_same_report_on_both_ranks(tmp_path):
    """Two ranks over gloo on this GPU: each checks on its replicated columns, no communication."""
    c, _ = CC.free_circuit()
    col, row = CC.FIRST
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "copy_constraints_worker.py"), str(tmp_path), str(col), str(row)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    want = [CC.check(c.sigmas, v, c.log_n, c.non_residues) for v in (c.variables, CC.changed(c.variables, col, row))]
    assert [w.kind for w in want] == [0, 3]
    for rank in range(2):
        with open(os.path.join(str(tmp_path), "reports_%d.json" % rank)) as f:
            got = json.load(f)
        assert [tuple(g[:8]) + (tuple(g[8]),) for g in got] == [w.fields() for w in want], "rank %d" % rank
