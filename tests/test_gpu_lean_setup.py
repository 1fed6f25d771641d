"""-m gpu: lean setups (BJ_SETUP_LEAN).  A lean setup drops the LDE of its columns once its tree stands; a proof then
rebuilds the quotient's cosets from the monomials one at a time and EVALUATES the setup words of the queried leaves
(eval_monomials_at_kernel, csrc/openings.hip).  The contract is byte identity: every case builds the same circuit twice in one
process and one context, resident and lean, and compares caps, proofs and reports word for word — no oracle of its own."""
import contextlib
import functools
import os

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding, proof_format, synthetic as S
from gpu_util import ctx

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def switch(value):
    """BJ_SETUP_LEAN = value (None: unset) as the library reads it, for the block; never while a proof runs."""
    lib = ctx()._lib        # the context first: it brings the HIP runtime in the order this process needs (gpu_util.ctx)
    before = os.environ.get("BJ_SETUP_LEAN")
    try:
        if value is None:
            os.environ.pop("BJ_SETUP_LEAN", None)
        else:
            os.environ["BJ_SETUP_LEAN"] = value
        lib.bj_env_reload()
        yield
    finally:
        if before is None:
            os.environ.pop("BJ_SETUP_LEAN", None)
        else:
            os.environ["BJ_SETUP_LEAN"] = before
        lib.bj_env_reload()


def pair(c, *args, **kw):
    """(resident, lean) setups of one circuit and one config, each created under its own value of the switch."""
    with switch(None):
        r = E.ProverSetup(ctx(), c, *args, **kw)
    with switch("1"):
        l = E.ProverSetup(ctx(), c, *args, **kw)
    return r, l


def setup_lde_bytes(s):
    c = s.circuit
    n_cols = c.num_vars + c.num_constant_cols + (c.tables.shape[0] if c.lookup_reps else 0)   # sigma || constants || tables
    return n_cols * max(s.fri_lde_factor, c.quotient_degree) * c.n * 8


def assert_same_proofs(r, l, sec):
    """Bytes (item 1 of the issue), then proofs word for word, and bj_verify_proof on the lean setup's own handle."""
    assert l.device_bytes() == r.device_bytes() - setup_lde_bytes(r)
    assert np.array_equal(r.cap(), l.cap())
    pr, _ = r.prove()
    vk = l.verifier()
    try:
        pl, report = l.prove_verified(vk)
    finally:
        vk.close()
    assert pr.shape == pl.shape and np.array_equal(pr, pl), "first differing word: %s" % (np.nonzero(pr != pl)[0][:4] if pr.shape == pl.shape else "sizes")
    assert report.stage == binding.VERIFY_OK and report.queries_checked == len(proof_format.parse(pl, security_level=sec)["_query_indices"])
    return pl


CASES = {
    # 2^8 rows: one coefficient per lane of the evaluation kernel's workgroup; L = q > fri_lde
    "2p8_q_above_fri": (lambda: S.sha_shaped_circuit(8, seed=108, table_bits=2), (2, 4, 20), {}),
    "2p7_fewer_coefficients_than_lanes": (lambda: S.sha_shaped_circuit(7, seed=107, table_bits=1), (8, 16, 20), {}),
    "2p12_plan_L12": (lambda: S.sha_shaped_circuit(12, seed=112, table_bits=2), (8, 16, 40), {}),
    "2p13_plan_R1_L12": (lambda: S.sha_shaped_circuit(13, seed=113, table_bits=2, num_gp_vars=20, lookup_width=4, lookup_reps=1,
                                                      mix=(0.2, 0.2, 0.2)), (8, 8, 60), {}),
    "2p14_plan_F4_L10": (lambda: S.sha_shaped_circuit(14, seed=114, table_bits=4), (4, 16, 50), {}),
    "table_id_variable": (lambda: S.sha_shaped_circuit(10, seed=710, table_bits=2, table_id_as_variable=True), (8, 16, 30), {}),
    "specialized_columns_own_constants": (lambda: S.sha_shaped_circuit(12, seed=712, table_bits=2, table_id_as_variable=True, boolean_columns=2,
                                                                       specialized_constant_columns=3), (8, 16, 30), {}),
    "specialized_columns_table_id_constant": (lambda: S.sha_shaped_circuit(10, seed=33, table_bits=2, boolean_columns=2,
                                                                           specialized_constant_columns=3), (8, 16, 30), {}),
    "witness_columns": (lambda: S.sha_shaped_circuit(10, seed=5, table_bits=2, gates=S.witness_gates(60, 4, 5), mix=(0.05, 0.3, 0.3, 0.2),
                                                     num_witness_cols=5), (8, 16, 30), {}),
    "poseidon2_flattened_gate": (lambda: S.recursion_like_circuit(10, seed=4), (8, 16, 30), {}),
    "blake2s_pairing": (lambda: S.sha_shaped_circuit(9, seed=72, table_bits=2), (8, 16, 40), dict(transcript="blake2s")),
    "pow": (lambda: S.sha_shaped_circuit(9, seed=70, table_bits=2), (8, 16, 40), dict(pow_bits=10)),
    "q_below_fri": (lambda: S.sha_shaped_circuit(9, seed=63, table_bits=2), (16, 32, 40), {}),
    "q_equals_fri": (lambda: S.sha_shaped_circuit(9, seed=64, table_bits=2, num_gp_vars=60, lookup_width=3, lookup_reps=8, num_public_inputs=1),
                     (4, 4, 20), {}),
    "more_queries_than_cap_nodes": (lambda: S.sha_shaped_circuit(8, seed=65, table_bits=2), (2, 4, 60), {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lean_proof_is_the_resident_proof(name):
    """Items 1 and 2 of the issue.  The geometries: 2^7 and 2^8 rows (fewer coefficients than lanes, and one each), the first
    non-generic transform plans (2^12: L12, 2^13: R1 L12, 2^14 with 16-byte aligned columns: F4 L10), the table id as a constant and
    as a variable column, gates over specialized columns with per-repetition constants, non-copiable witness columns, the Poseidon2
    and Blake2s pairings, PoW, quotient degree above, below and equal to the FRI LDE factor, and 60 queries into 512 leaves under 4 cap
    nodes (queries repeat leaves or land next to each other)."""
    make, (fri_lde, cap, sec), kw = CASES[name]
    c = make()
    if name == "2p8_q_above_fri":
        assert c.quotient_degree > fri_lde
    if name == "q_below_fri":
        assert c.quotient_degree < fri_lde
    if name == "q_equals_fri":
        assert c.quotient_degree == fri_lde
    r, l = pair(c, fri_lde, cap, sec, **kw)
    try:
        assert l.lean is False and r.lean is False      # the property tells what the constructor was asked, the bytes tell the rest
        pl = assert_same_proofs(r, l, sec)
        if name == "more_queries_than_cap_nodes":
            idx = proof_format.parse(pl, security_level=sec)["_query_indices"]
            assert len(idx) > cap and len(idx) >= 30
    finally:
        r.close()
        l.close()


def test_lean_keyword_of_the_binding():
    """ProverSetup(lean=True) makes the same setup as the switch does and leaves the environment as it found it."""
    c = S.sha_shaped_circuit(9, seed=90, table_bits=2)
    with switch(None):
        r = E.ProverSetup(ctx(), c, 8, 16, 30)
        l = E.ProverSetup(ctx(), c, 8, 16, 30, lean=True)
        assert "BJ_SETUP_LEAN" not in os.environ
        r2 = E.ProverSetup(ctx(), c, 8, 16, 30)         # the library read the restored value: resident again
    with switch("0"):
        r3 = E.ProverSetup(ctx(), c, 8, 16, 30)         # "0" is off, as for the other switches
    try:
        assert l.lean and not r.lean
        assert r2.device_bytes() == r.device_bytes() == r3.device_bytes()
        assert_same_proofs(r, l, 30)
        with pytest.raises(E.BoojumHipError, match="single-GPU"):
            E.ProverSetup(ctx(), c, 8, 16, 30, lean=True, comm=object())
    finally:
        for s in (r, l, r2, r3):
            s.close()


def test_first_and_last_leaf():
    """Item 3: the evaluation kernel at leaf 0 (x = 7, the coset shift itself) and at leaf N - 1.  Which leaves a proof queries is up
    to its transcript; the kernel-level test asserts those two leaves directly, at every size and layout
    (tests/test_gpu_prover_only_kernels.py: Context.eval_monomials_at against the definition and the oracle's LDE, leaf 0 and
    leaf N - 1 in every index set).  Here: one resident / lean pair of this geometry (2^8 rows, 60 queries into 512 leaves) — the
    lean proof is the resident proof word for word, and it verifies."""
    fri_lde, cap, sec = 2, 4, 60
    r, l = pair(S.sha_shaped_circuit(8, seed=1000, table_bits=2), fri_lde, cap, sec)
    try:
        idx = proof_format.parse(assert_same_proofs(r, l, sec), security_level=sec)["_query_indices"]
        assert len(idx) >= 30 and all(0 <= i < (fri_lde << 8) for i in idx)
    finally:
        r.close()
        l.close()


def test_resident_and_lean_setups_coexist():
    """Item 4: two circuits, one setup resident and one lean, four proofs interleaved with the switch flipped in between: a setup's
    mode is what the switch was when it was created, whatever the switch says when it proves."""
    ca, cb = S.sha_shaped_circuit(10, seed=41, table_bits=2), S.sha_shaped_circuit(9, seed=42, table_bits=2, table_id_as_variable=True)
    ra, la = pair(ca, 8, 16, 30)
    rb, lb = pair(cb, 4, 8, 30)
    try:
        with switch(None):
            ref_a, ref_b = ra.prove()[0], rb.prove()[0]
        bytes_before = (ra.device_bytes(), lb.device_bytes())
        with switch("1"):
            p1 = ra.prove()[0]          # resident setup, switch on
        with switch(None):
            p2 = lb.prove()[0]          # lean setup, switch off
        with switch("1"):
            p3 = lb.prove()[0]
            p4 = ra.prove()[0]
        with switch(None):
            p5, p6 = la.prove()[0], rb.prove()[0]
        assert all(np.array_equal(p, ref_a) for p in (p1, p4, p5)) and all(np.array_equal(p, ref_b) for p in (p2, p3, p6))
        assert (ra.device_bytes(), lb.device_bytes()) == bytes_before
        assert lb.device_bytes() == rb.device_bytes() - setup_lde_bytes(rb) and la.device_bytes() == ra.device_bytes() - setup_lde_bytes(ra)
    finally:
        for s in (ra, la, rb, lb):
            s.close()


def test_other_consumers_of_a_setup():
    """Item 5: the satisfiability check (satisfied and broken witness: the same report), the multiplicity count (the same column),
    two asynchronous proofs in flight (the same bytes), the verification key (the same verdicts)."""
    c = S.sha_shaped_circuit(10, seed=55, table_bits=2)
    r, l = pair(c, 8, 16, 30)
    try:
        assert r.check_satisfied() == l.check_satisfied() and l.check_satisfied()
        bad = c.variables.copy()
        rows = np.nonzero(c.constants[0] == 1)[0]
        bad[3, rows[0]] = (int(bad[3, rows[0]]) + 1) % E.P
        assert r.check_satisfied(variables=bad) == l.check_satisfied(variables=bad) and not l.check_satisfied(variables=bad)
        assert np.array_equal(r.count_multiplicities(), l.count_multiplicities())
        d_vars = ctx().upload(c.variables)
        try:
            assert r.check_copy_constraints(d_vars) == l.check_copy_constraints(d_vars) and l.check_copy_constraints(d_vars)
            ref, _ = r.prove()
            counted, _ = l.prove_dev(d_vars, None, count_multiplicities=True)
            assert np.array_equal(counted, ref)
        finally:
            ctx().free(d_vars)
        t1, t2 = l.prove_async(), l.prove_async()
        a1, a2 = l.wait(t1)[0], l.wait(t2)[0]
        assert np.array_equal(a1, ref) and np.array_equal(a2, ref)
        assert r.verify(ref) and l.verify(ref)
        broken = ref.copy()
        broken[-1] ^= np.uint64(1)
        assert str(r.verify(broken)) == str(l.verify(broken)) and not l.verify(broken)
    finally:
        r.close()
        l.close()
        ctx().release_workspace()


@functools.lru_cache(maxsize=None)
def _real_sha():
    from era_boojum_amd import sha256_circuit as SHA
    return SHA.sha256_circuit(SHA.bench_message(33, seed=3), return_info=True)


def test_dumps_on_a_lean_placement_setup():
    """Item 5, last line: bj_prove_from_dumps with no hint on a lean bj_setup_create_from_placement setup; the placement stays, the
    LDE goes."""
    from era_boojum_amd import memcopy_format as M
    from era_boojum_amd import sha256_circuit as SHA
    c, info = _real_sha()
    with switch(None):
        r = E.ProverSetup.from_placement(ctx(), c, info["var_ids"], 8, 16, 30)
    with switch("1"):
        l = E.ProverSetup.from_placement(ctx(), c, info["var_ids"], 8, 16, 30)
    try:
        assert l.device_bytes() == r.device_bytes() - setup_lde_bytes(r) and np.array_equal(r.cap(), l.cap())
        total = sum(t.shape[0] for t in SHA.sha_tables())
        wit = M.write_witness_vec([(col, row) for col, row, _ in c.public_inputs], info["all_values"], c.multiplicities[0, :total].astype(np.uint32))
        want, _ = r.prove_from_dumps(wit, None)
        got, _ = l.prove_from_dumps(wit, None)
        assert np.array_equal(want, got)
        assert r.check_satisfied_from_dumps(wit, None) == l.check_satisfied_from_dumps(wit, None)
        # and the setup made from the reference's SetupBaseStorage dump honours the switch too
        with switch("1"):
            d = E.ProverSetup(ctx(), c, 8, 16, 30, setup_base_dump=M.write_setup_base(c))
        try:
            assert d.device_bytes() == l.device_bytes() - 4 * c.num_vars * c.n
            assert np.array_equal(d.prove()[0], r.prove()[0])
        finally:
            d.close()
    finally:
        r.close()
        l.close()


def test_workspace_of_a_lean_proof():
    """Item 6: a lean proof reserves one coset of the setup columns more than the resident proof of the same circuit — the evaluation
    kernel writes into the query block both proofs have, so nothing is added for it — and with the switch off ("0" or unset) the
    reservation is the same number."""
    c = S.sha_shaped_circuit(11, seed=66, table_bits=2)
    r, l = pair(c, 8, 16, 30)
    with switch("0"):
        r0 = E.ProverSetup(ctx(), c, 8, 16, 30)
    try:
        ws = []
        for s in (r, r0, l):
            ctx().release_workspace()       # the arena only grows: start every measurement from none
            s.prove()
            ws.append(dict(s.last_workspace))
        ctx().release_workspace()
        coset = setup_lde_bytes(r) // max(r.fri_lde_factor, c.quotient_degree)
        print("workspace bytes: resident %s, switch=0 %s, lean %s, one coset %d" % (ws[0], ws[1], ws[2], coset))
        assert ws[0] == ws[1]
        for k in ("reserved_bytes", "high_water_bytes"):
            assert ws[0][k] < ws[2][k] <= ws[0][k] + coset
        assert all(w["overflow_slabs"] == 0 for w in ws)
    finally:
        for s in (r, r0, l):
            s.close()


def test_tiled_monomials_at_2p22_rows():
    """Item 7: 2^22 rows, where the monomials lie in the tiled layout and the evaluation kernel reads them through its index map.
    Ten general-purpose columns, no lookups: the narrowest geometry the prover takes (more columns than the quotient degree).
    Measured on an MI355X: 2.3 s for the whole test, most of it the synthesis of the circuit on the host."""
    assert ctx().monomials_tiled(22)
    c = S.sha_shaped_circuit(22, seed=22, table_bits=2, num_gp_vars=10, lookup_width=1, lookup_reps=1, num_public_inputs=1)
    c.variables = np.ascontiguousarray(c.variables[:c.num_gp_vars]); c.sigmas = np.ascontiguousarray(c.sigmas[:c.num_gp_vars])
    c.non_residues = c.non_residues[:c.num_gp_vars]
    c.constants = np.ascontiguousarray(c.constants[:c.num_constants_for_gates]); c.num_constant_cols = c.num_constants_for_gates
    c.num_lookup_vars = 0; c.lookup_reps = 0
    r, l = pair(c, 2, 4, 20)
    try:
        assert l.device_bytes() == r.device_bytes() - setup_lde_bytes(r) and np.array_equal(r.cap(), l.cap())
        d_vars = ctx().upload(c.variables)
        try:
            pr, _ = r.prove_dev(d_vars, None)
            pl, _ = l.prove_dev(d_vars, None)
        finally:
            ctx().free(d_vars)
        assert np.array_equal(pr, pl)
        assert l.verify(pl)
    finally:
        r.close()
        l.close()
        ctx().release_workspace()
