"""-m gpu: lean proofs (BJ_PROOF_LEAN).  A lean proof keeps the monomials and the trees of its witness and stage-2
oracles and ONE coset of each: every coset under the trees is extended and hashed in turn, the quotient's cosets are extended
again, every opening set is combined on its monomials, and the witness and stage-2 words of the queried leaves are evaluated
(eval_monomials_at_kernel).  The contract is byte identity: every case proves one setup twice in one process and one context, with
the switch off and on, and compares the proofs word for word — no oracle of its own.

The mode has no entry point of its own: tests/test_verify_batch_host.py pins the number of entry points, so the switch is the
environment's (era_boojum_amd.binding.lean_proofs sets it and has the library read it), as BJ_SETUP_LEAN is."""
import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding, proof_format, synthetic as S
from gpu_util import ctx

pytestmark = pytest.mark.gpu


def lean(on=True):
    return ctx().lean_proofs(on)


def setup_lean():
    """BJ_SETUP_LEAN for the block, as ProverSetup(lean=True) does it."""
    return binding._setup_lean_switch(ctx()._lib, True)


def on_device(s, fn):
    """fn(d_variables, d_multiplicities) with the witness of s's circuit resident (the non-copiable columns behind the variables)."""
    v, m, _ = s._host_witness(None, None, None)
    d_v, d_m = ctx().upload(v), ctx().upload(m)
    try:
        return fn(d_v, d_m)
    finally:
        ctx().free(d_v)
        ctx().free(d_m)


def same(a, b):
    assert a.shape == b.shape and np.array_equal(a, b), "first differing word: %s" % (np.nonzero(a != b)[0][:4] if a.shape == b.shape else "sizes")


def resident_then_lean(s, sec):
    """bj_prove and bj_prove_dev with the switch off, then both with it on; the lean bj_prove is checked by bj_verify_proof.
    Returns the proof."""
    with lean(False):
        ref, _ = s.prove()
        same(on_device(s, lambda v, m: s.prove_dev(v, m)[0]), ref)
    vk = s.verifier()
    try:
        with lean():
            got, report = s.prove_verified(vk)
            dev = on_device(s, lambda v, m: s.prove_dev(v, m)[0])
    finally:
        vk.close()
    same(got, ref)
    same(dev, ref)
    assert report.stage == binding.VERIFY_OK
    assert report.queries_checked == len(proof_format.parse(got, security_level=sec)["_query_indices"])
    return got


# the geometries of the lean-setup tests (tests/test_gpu_lean_setup.py::CASES), restated: they were chosen for the same kernels
CASES = {
    # 2^8 rows: one coefficient per lane of the evaluation kernel's workgroup; L = q > fri_lde: the quotient reads more cosets than the trees cover
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
    # q < fri_lde: the trees cover more cosets than the quotient reads
    "q_below_fri": (lambda: S.sha_shaped_circuit(9, seed=63, table_bits=2), (16, 32, 40), {}),
    # one public input on a variable column: its row set goes through the monomials although it holds one column
    "q_equals_fri": (lambda: S.sha_shaped_circuit(9, seed=64, table_bits=2, num_gp_vars=60, lookup_width=3, lookup_reps=8, num_public_inputs=1),
                     (4, 4, 20), {}),
    "more_queries_than_cap_nodes": (lambda: S.sha_shaped_circuit(8, seed=65, table_bits=2), (2, 4, 60), {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_lean_proof_is_the_resident_proof(name):
    make, (fri_lde, cap, sec), kw = CASES[name]
    c = make()
    if name == "2p8_q_above_fri":
        assert c.quotient_degree > fri_lde
    if name == "q_below_fri":
        assert c.quotient_degree < fri_lde
    if name == "q_equals_fri":
        assert c.quotient_degree == fri_lde and len(c.public_inputs) == 1 and c.public_inputs[0][0] < c.num_vars
    s = E.ProverSetup(ctx(), c, fri_lde, cap, sec, **kw)
    try:
        p = resident_then_lean(s, sec)
        if name == "more_queries_than_cap_nodes":
            idx = proof_format.parse(p, security_level=sec)["_query_indices"]
            assert len(idx) > cap and len(idx) >= 30
    finally:
        s.close()


def test_setup_and_proof_lean_or_resident_in_all_four_combinations():
    """Setup {resident, lean} x proof {resident, lean} on one circuit with lookups and a public input: four identical proofs.  The
    quotient loop takes each oracle's coset from its LDE or rebuilds it, independently."""
    c = S.sha_shaped_circuit(10, seed=44, table_bits=2, num_public_inputs=1)
    r = E.ProverSetup(ctx(), c, 8, 16, 30)
    with setup_lean():
        l = E.ProverSetup(ctx(), c, 8, 16, 30)
    try:
        assert l.device_bytes() < r.device_bytes()
        with lean(False):
            ref = r.prove()[0]
            same(l.prove()[0], ref)
        with lean():
            same(r.prove()[0], ref)
            same(l.prove()[0], ref)
            same(on_device(l, lambda v, m: l.prove_dev(v, m)[0]), ref)
        assert r.verify(ref)
    finally:
        r.close()
        l.close()


@pytest.mark.parametrize("transcript", ["poseidon2", "blake2s"])
def test_host_witness(transcript):
    """bj_prove in lean mode: on a Poseidon2 setup, whose resident proof absorbs the column groups into the leaf sponges as they land
    (a lean proof hashes coset by coset after the last group), and on a Blake2s setup, which never did.  More columns than one
    group of eight, so that the copies and the inverse transforms do run in groups."""
    c = S.sha_shaped_circuit(11, seed=81, table_bits=2)
    assert c.num_vars > 16
    kw = {} if transcript == "poseidon2" else dict(transcript=transcript)
    s = E.ProverSetup(ctx(), c, 8, 16, 30, **kw)
    try:
        with lean(False):
            ref = s.prove()[0]
        with lean():
            same(s.prove()[0], ref)
        assert s.verify(ref)
    finally:
        s.close()


def test_multiplicities_counted_on_the_device():
    """NULL multiplicities: the column is counted into the arena (bj_prove_dev) or the staging (bj_prove) before round 1 transforms it."""
    c = S.sha_shaped_circuit(10, seed=55, table_bits=2)
    s = E.ProverSetup(ctx(), c, 8, 16, 30)
    try:
        with lean(False):
            ref = s.prove()[0]
        with lean():
            same(on_device(s, lambda v, m: s.prove_dev(v, None, count_multiplicities=True)[0]), ref)
            same(s.prove(count_multiplicities=True)[0], ref)
    finally:
        s.close()


def test_first_and_last_leaf():
    """The witness and stage-2 words at leaf 0 (x = 7, the coset shift itself) and at leaf N - 1.  Which leaves a proof queries is up
    to its transcript: 60 queries into the 256 leaves of a 2^7-row trace at LDE 2 reach one of the two with probability 0.37 per
    circuit, so the seeds are searched, at most 16 of them, for the first whose resident proof queries leaf 0 or leaf N - 1; that
    proof is then made lean.  Were there none, the assertion is on the smallest and largest leaf reached by the last seed."""
    fri_lde, cap, sec, log_n = 2, 4, 60, 7
    N = fri_lde << log_n
    for seed in range(2000, 2016):
        s = E.ProverSetup(ctx(), S.sha_shaped_circuit(log_n, seed=seed, table_bits=1), fri_lde, cap, sec)
        try:
            with lean(False):
                ref = s.prove()[0]
            idx = [int(i) for i in proof_format.parse(ref, security_level=sec)["_query_indices"]]
            if not (0 in idx or N - 1 in idx) and seed != 2015:
                continue
            with lean():
                same(s.prove()[0], ref)
            assert s.verify(ref)
            print("seed %d: %d queries, smallest leaf %d, largest %d of %d" % (seed, len(idx), min(idx), max(idx), N))
            assert len(idx) >= 30 and 0 <= min(idx) and max(idx) < N
            assert 0 in idx or N - 1 in idx, "no seed in 2000..2015 queried leaf 0 or leaf N - 1: smallest %d, largest %d" % (min(idx), max(idx))
            return
        finally:
            s.close()


def test_async_lanes():
    """bj_prove_async with the switch on: the two lanes are sub-contexts and read the same switch when they take a proof up; two tickets
    in flight, each the serial resident proof.  (There is no per-context setter to call between submission and wait: see the
    module's docstring.)"""
    c = S.sha_shaped_circuit(10, seed=91, table_bits=2)
    s = E.ProverSetup(ctx(), c, 8, 16, 30)
    try:
        with lean(False):
            ref = s.prove()[0]
        with lean():
            t1, t2 = s.prove_async(), s.prove_async()
            a1, a2 = s.wait(t1)[0], s.wait(t2)[0]
        same(a1, ref)
        same(a2, ref)
    finally:
        s.close()
        ctx().release_workspace()


def test_arena_sizes():
    """After release_workspace() a lean proof reserves the smaller arena: reserved >= high-water, no overflow slab, and smaller than
    the resident proof's by at least ((nW + nS2) (Ln - n) - 2 N S) 8 bytes — what the two one-coset buffers save less one extended
    numerator per opening set (S of them: at z, at z omega, the lookup sums at 0, the public input's row).  Resident again: the arena
    grows through the path every larger proof takes, and the proof is still the same."""
    c = S.sha_shaped_circuit(11, seed=66, table_bits=2, num_public_inputs=1)
    fri_lde = 8
    s = E.ProverSetup(ctx(), c, fri_lde, 16, 30)
    try:
        ws = {}
        ctx().release_workspace()
        with lean(False):
            ref = on_device(s, lambda v, m: s.prove_dev(v, m)[0])
            ws["resident"] = dict(s.last_workspace)
        ctx().release_workspace()
        with lean():
            same(on_device(s, lambda v, m: s.prove_dev(v, m)[0]), ref)
            ws["lean"] = dict(s.last_workspace)
        with lean(False):
            same(on_device(s, lambda v, m: s.prove_dev(v, m)[0]), ref)
            ws["resident again"] = dict(s.last_workspace)
        with lean():                                   # the arena only grows: a lean proof in the larger one
            same(on_device(s, lambda v, m: s.prove_dev(v, m)[0]), ref)
            ws["lean again"] = dict(s.last_workspace)
        nW, nS2 = int(ref[10]), int(ref[11])           # the header's leaf widths (proof_layout.h, ProofHeader)
        q, V = c.quotient_degree, c.num_vars
        assert nW == V + 1 and nS2 == 2 * (1 + (-(-V // q) - 1) + c.lookup_reps + 1)
        n, L = c.n, max(fri_lde, q)
        N, Ln, sets = fri_lde * n, L * n, 4
        bound = ((nW + nS2) * (Ln - n) - 2 * N * sets) * 8
        print("workspace bytes: %s; bound %d" % (ws, bound))
        for w in ws.values():
            assert w["overflow_slabs"] == 0 and w["reserved_bytes"] >= w["high_water_bytes"]
        assert bound > 0 and ws["lean"]["reserved_bytes"] <= ws["resident"]["reserved_bytes"] - bound
        assert ws["lean"]["high_water_bytes"] <= ws["resident"]["high_water_bytes"] - bound
        assert ws["resident again"] == ws["resident"]
        assert ws["lean again"]["reserved_bytes"] == ws["resident"]["reserved_bytes"]
        assert ws["lean again"]["high_water_bytes"] == ws["lean"]["high_water_bytes"]
    finally:
        s.close()
        ctx().release_workspace()


def _plan_words(c, fri_lde, cap, sec, lean_proof):
    """Total words of the workspace plan (csrc/workspace_plan.h) of a bj_prove_dev proof of c on one GPU, through the host helper."""
    import ctypes as C
    from era_boojum_amd import build
    lib = C.CDLL(build.build_canon_helper())
    lib.bj_workspace_plan_summary.restype = None
    new_pow, nq, sched, _ = binding.fri_schedule(sec, cap, 0, fri_lde.bit_length() - 1, c.log_n)
    u = lambda xs: (C.c_uint * max(len(xs), 1))(*xs)
    nine = [c.log_n, c.num_vars, c.num_gp_vars, int(getattr(c, "num_witness_cols", 0)), c.num_constant_cols, c.lookup_width, c.lookup_reps,
            c.table_id_col, c.quotient_degree]
    # powers of the quotient challenge: lookup | gates | L1 | copy-permutation chunks (prover.hip, round 3)
    alpha_terms = c.lookup_reps + 1 + sum(g.reps * g.num_terms for g in c.gates) + 1 + -(-c.num_vars // c.quotient_degree)
    out = (C.c_size_t * 4)()
    lib.bj_workspace_plan_summary(u(nine), C.c_uint(fri_lde), C.c_uint(cap), C.c_uint(1), C.c_uint(alpha_terms),
                                  u([p[0] for p in c.public_inputs]), u([p[1] for p in c.public_inputs]), C.c_size_t(len(c.public_inputs)),
                                  u([4 if lean_proof else 0, 0, 0, int(new_pow != 0)]), (C.c_uint32 * 32)(*sched), C.c_size_t(len(sched)),
                                  C.c_size_t(nq), out)
    return int(out[0])


def test_same_probes_and_the_plan_of_each_mode():
    """What byte identity does not show: a resident and a lean proof of one 2^7-row circuit list the same kernel probes in the same
    order (bj_proof_kernel_stats), and each reserves exactly the total of the workspace plan of its mode (bj_proof_workspace_bytes
    in a context whose workspace was released: the reservation IS the plan's total)."""
    fri_lde, cap, sec = 8, 16, 20
    c = S.sha_shaped_circuit(7, seed=107, table_bits=1)
    assert c.lookup_reps > 0 and c.public_inputs and not c.specialized_gates   # every kind of opening set; no terms but the gates', lookups' and chunks'
    s = E.ProverSetup(ctx(), c, fri_lde, cap, sec)
    try:
        probes, proofs = {}, {}
        for mode in (False, True):
            ctx().release_workspace()
            with lean(mode):
                proofs[mode] = on_device(s, lambda v, m: s.prove_dev(v, m)[0])
            probes[mode] = list(s.last_kernels)
            ws, plan = dict(s.last_workspace), _plan_words(c, fri_lde, cap, sec, mode)
            print("lean %s: probes %s; reserved %d bytes, plan %d words" % (mode, probes[mode], ws["reserved_bytes"], plan))
            assert ws["overflow_slabs"] == 0 and ws["reserved_bytes"] == 8 * plan
        same(proofs[True], proofs[False])
        assert len(probes[False]) >= 2 and probes[True] == probes[False]
    finally:
        s.close()
        ctx().release_workspace()


def test_tiled_monomials_at_2p22_rows():
    """2^22 rows, the one size where mono and mono_s2 lie in the tiled layout: the per-coset extension reads it, and the evaluation
    kernel reads it in place through its index map.  The circuit of the lean-setup test of this size: ten general-purpose columns,
    no lookups, one public input.  Resident against lean proof, word for word."""
    assert ctx().monomials_tiled(22)
    c = S.sha_shaped_circuit(22, seed=22, table_bits=2, num_gp_vars=10, lookup_width=1, lookup_reps=1, num_public_inputs=1)
    c.variables = np.ascontiguousarray(c.variables[:c.num_gp_vars]); c.sigmas = np.ascontiguousarray(c.sigmas[:c.num_gp_vars])
    c.non_residues = c.non_residues[:c.num_gp_vars]
    c.constants = np.ascontiguousarray(c.constants[:c.num_constants_for_gates]); c.num_constant_cols = c.num_constants_for_gates
    c.num_lookup_vars = 0; c.lookup_reps = 0
    s = E.ProverSetup(ctx(), c, 2, 4, 20)
    try:
        d_vars = ctx().upload(c.variables)
        try:
            with lean(False):
                pr, _ = s.prove_dev(d_vars, None)
            with lean():
                pl, _ = s.prove_dev(d_vars, None)
        finally:
            ctx().free(d_vars)
        same(pr, pl)
        assert s.verify(pl)
    finally:
        s.close()
        ctx().release_workspace()
