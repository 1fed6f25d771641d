"""-m gpu: bj_list_unsatisfied (csrc/list_unsatisfied.hip) against the exact restatement tests/unsat_list_ref.py, entry by entry
and field by field: satisfied circuits, one wrong cell at every wave and block edge of the compaction (rows 511 and 512 of seams10
select NopGate, where no gate term can fail: their wrong cell is a looked-up one), a dense family under every capacity (the small
ones take the chunked counting path: 256 rows per chunk at 2^10 rows), both gate kinds with lookups and multiplicities cut inside
kind 2 and inside kind 3, non-canonical cells, the from-dumps form, agreement with bj_check_satisfied, neutrality towards proofs,
the argument errors, determinism."""
import ctypes as C
import functools

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding
from gpu_util import ctx

import satisfiability_cases as K
import unsat_list_cases as U
import unsat_list_ref as L

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def setup(name):
    return E.ProverSetup(ctx(), K.circuit(name), 8, 16, 30)


def agree(s, full, mult, want, capacity):
    """The GPU list at `capacity` is the first min(capacity, total) entries of `want`, the totals are the whole list's."""
    want_entries, want_totals = want
    entries, totals = s.list_unsatisfied(full, mult, capacity=capacity)
    assert totals == want_totals
    assert len(entries) == min(capacity, want_totals[0])
    assert [e.fields() for e in entries] == want_entries[:capacity]
    return entries


def agree_case(name, capacity=None):
    cname, full, mult = U.case(name)
    want = U.reference(name)
    return agree(setup(cname), full, mult, want, want[1][0] + 3 if capacity is None else capacity)


@pytest.mark.parametrize("name", K.SATISFIED)
def test_satisfied_circuits(name):
    s = setup(name)
    for capacity in (0, 16):
        assert s.list_unsatisfied(capacity=capacity) == ([], (0, 0, 0, 0, 0))


@pytest.mark.parametrize("name", ["edges"] + ["edge_%d" % i for i in range(len(U.EDGE_ROWS))])
def test_wave_and_block_edges(name):
    entries = agree_case(name)
    if name != "edges":
        row = U.EDGE_ROWS[int(name[5:])] % K.circuit("seams10").n
        assert entries[0].row == row and entries[0].kind in (binding.UNSAT_GATE, binding.UNSAT_LOOKUP)


def test_dense_family_under_every_capacity():
    total = U.reference("dense")[1][0]
    assert 512 < total < 1000          # several blocks of flagged rows; 1000 and the last capacity hold the whole list
    for capacity in (0, 1, 7, 64, 65, 1000, total + 100):
        agree_case("dense", capacity)


@pytest.mark.parametrize("name", ["mixed_spec10", "mixed_tidvar13"])
def test_both_gate_kinds_and_lookups_in_one_witness(name):
    t = U.reference(name)[1]
    assert t[2] >= 2 and t[3] == 2 and t[4] >= 1
    inside_2, inside_3, before_4, all_of_it = t[1] + 1, t[1] + t[2] + 1, t[1] + t[2] + t[3], t[0]
    assert agree_case(name, inside_2)[-1].kind == binding.UNSAT_SPECIALIZED_GATE
    assert agree_case(name, inside_3)[-1].kind == binding.UNSAT_LOOKUP
    assert all(e.kind != binding.UNSAT_MULTIPLICITY for e in agree_case(name, before_4))
    assert [e.kind for e in agree_case(name, before_4 + 1)].count(binding.UNSAT_MULTIPLICITY) == 1
    assert [e.kind for e in agree_case(name, all_of_it)].count(binding.UNSAT_MULTIPLICITY) == t[4]


def test_many_terms_of_one_row():
    agree_case("poseidon_row")
    agree_case("poseidon_row", 5)


@pytest.mark.parametrize("name", ["edges", "mixed_tidvar13", "poseidon_row"])
def test_noncanonical_cells_give_the_same_list(name):
    cname, full, mult = U.case(name)
    nc = K.noncanonical(full)
    assert np.any(nc != full)
    want = U.reference(name)
    agree(setup(cname), nc, K.noncanonical(mult), want, want[1][0])


def test_from_dumps():
    from era_boojum_amd import memcopy_format as M
    s = setup("witness10")
    c = s.circuit
    V, n, Wc = c.num_vars, c.n, c.num_witness_cols
    all_values = np.concatenate([c.variables.reshape(-1), c.witness.reshape(-1)])
    var_ids = np.arange(V * n, dtype=np.int64).reshape(V, n)
    wit_ids = V * n + np.arange(Wc * n, dtype=np.int64).reshape(Wc, n)
    pubs = [(col, row) for col, row, _ in c.public_inputs]
    mult = c.multiplicities[0, :c.total_tables_len].astype(np.uint32)
    hints = (M.write_variables_hint(var_ids), M.write_variables_hint(wit_ids))
    assert s.list_unsatisfied_from_dumps(M.write_witness_vec(pubs, all_values, mult), *hints) == ([], (0, 0, 0, 0, 0))
    gi = K.gate_index(c, "ZeroCheckGate[witness]")
    broken = all_values.copy()
    for row in K.gate_rows(c, gi)[3:6]:
        cell = V + (c.gates[gi].reps - 1) * c.gates[gi].wit_stride          # the inverse in the last repetition's witness column
        broken[cell * n + row] = (int(broken[cell * n + row]) + 1) % E.P
    want = L.listing(c, broken.reshape(V + Wc, n))
    assert want[1][1] >= 3
    for capacity in (2, 64):
        got = s.list_unsatisfied_from_dumps(M.write_witness_vec(pubs, broken, mult), *hints, capacity=capacity)
        assert got == s.list_unsatisfied(broken.reshape(V + Wc, n), capacity=capacity)
        assert [e.fields() for e in got[0]] == want[0][:capacity] and got[1] == want[1]
    with pytest.raises(E.BoojumHipError, match="invalid.*bj_list_unsatisfied_from_dumps: null argument"):
        s._ctx._check(s._lib.bj_list_unsatisfied_from_dumps(s._ctx._h, s._h, b"", 0, None, 0, None, 0, None, 4, None, None))


@pytest.mark.parametrize("name", U.PLANTED)
def test_entry_zero_is_the_report_of_check_satisfied(name):
    cname, full, mult = U.case(name)
    s = setup(cname)
    rep = s.check_satisfied(full, mult)
    entries, totals = s.list_unsatisfied(full, mult, capacity=1)
    assert len(entries) == 1
    assert entries[0].fields() == (rep.kind, rep.gate, rep.repetition, rep.term, rep.row, rep.value, rep.expected)
    assert totals[3:] == rep.failures[3:] and totals[1] >= rep.failures[1] and totals[2] >= rep.failures[2]


def test_a_listing_does_not_disturb_proofs():
    cname, bad, mult = U.case("mixed_spec10")
    s = setup(cname)
    c, c_ = s.circuit, s._ctx
    good = K.full_witness(c)
    d_good, d_bad, d_m, d_bad_m = c_.upload(good), c_.upload(bad), c_.upload(c.multiplicities), c_.upload(mult)
    try:
        before, _ = s.prove_dev(d_good, d_m)
        assert s.list_unsatisfied_dev(d_good, d_m, 8) == ([], (0, 0, 0, 0, 0))
        entries, totals = s.list_unsatisfied_dev(d_bad, d_bad_m, 64)
        assert ([e.fields() for e in entries], totals) == U.reference("mixed_spec10")
        after, _ = s.prove_dev(d_good, d_m)
        assert np.array_equal(before, after)
        assert np.array_equal(c_.d2h(d_good, good.shape), good) and np.array_equal(c_.d2h(d_bad, bad.shape), bad)
        assert np.array_equal(c_.d2h(d_bad_m, mult.shape), mult)
    finally:
        for p in (d_good, d_bad, d_m, d_bad_m):
            c_.free(p)


def _raw(s, d_v, d_m, capacity, entries=True, n_out=True, totals_out=True):
    buf = (binding._UnsatEntry * max(capacity, 1))()
    n, totals = C.c_size_t(77), (C.c_uint64 * 5)()
    rc = s._lib.bj_list_unsatisfied(s._ctx._h, s._h, d_v, d_m, buf if entries else None, capacity, C.byref(n) if n_out else None,
                                    totals if totals_out else None)
    return rc, bytes(buf), n.value, tuple(totals)


def test_argument_errors():
    s = setup("sha10")
    c = s.circuit
    h = s._ctx._h
    d_v, d_m = ctx().upload(c.variables), ctx().upload(c.multiplicities)
    try:
        assert _raw(s, d_v, d_m, 4, n_out=False)[0] == -1
        assert _raw(s, d_v, d_m, 4, totals_out=False)[0] == -1
        assert _raw(s, d_v, d_m, 4, entries=False)[0] == -1
        assert b"bj_list_unsatisfied: null argument" in s._lib.bj_last_error(h)
        assert _raw(s, None, d_m, 4)[0] == -1
        assert _raw(s, d_v, None, 4)[0] == -1
        assert b"multiplicities required" in s._lib.bj_last_error(h)
        assert _raw(s, d_v, d_m, 0, entries=False)[0::2] == (0, 0)            # a pure count
        assert _raw(s, d_v, d_m, 4)[2:] == (0, (0, 0, 0, 0, 0))
    finally:
        ctx().free(d_v)
        ctx().free(d_m)


def test_a_setup_without_lookups_ignores_multiplicities():
    """bj_check_satisfied takes NULL or any column there; so does the listing."""
    from era_boojum_amd import synthetic as S
    c = S.sha_shaped_circuit(10, seed=11, table_bits=2, lookup_reps=0)
    s = E.ProverSetup(ctx(), c, 8, 16, 30)
    full, _ = K.plant_gate(c, 1, int(K.gate_rows(c, 1)[0]))
    want = L.listing(c, full)
    d_good, d_bad, d_m = ctx().upload(K.full_witness(c)), ctx().upload(full), ctx().upload(np.ones((1, c.n), dtype=np.uint64))
    try:
        assert _raw(s, d_good, d_m, 4)[0::2] == (0, 0) and _raw(s, d_good, None, 4)[0::2] == (0, 0)
        assert s.check_satisfied_dev(d_bad, d_m).kind == binding.UNSAT_GATE
        for m in (d_m, None):
            entries, totals = s.list_unsatisfied_dev(d_bad, m, 4)
            assert ([e.fields() for e in entries], totals) == want and totals == (1, 1, 0, 0, 0)
    finally:
        for p in (d_good, d_bad, d_m):
            ctx().free(p)
        s.close()


def test_two_calls_return_the_same_bytes():
    cname, full, mult = U.case("dense")
    s = setup(cname)
    d_v, d_m = ctx().upload(full), ctx().upload(mult)
    try:
        for capacity in (65, 2000):
            a, b = _raw(s, d_v, d_m, capacity), _raw(s, d_v, d_m, capacity)
            assert a[0] == 0 and a == b and a[2] == min(capacity, U.reference("dense")[1][0])
    finally:
        ctx().free(d_v)
        ctx().free(d_m)
