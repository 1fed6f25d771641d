"""bj_verify (csrc/verifier.hip, csrc/verify_open.h): the product's own verifier against the proofs bj_prove emits, against
oracle/verifier.py on edited proofs — stage by stage — and against the reference's own proof (tests/golden)."""
import copy

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, proof_format, synthetic as S
from gpu_util import ctx
from verify_util import SWEEP_CLASSES, Layout, P, bump, fri_value_edit, golden_circuit, golden_config, golden_proof_dict, sweep_positions

pytestmark = pytest.mark.gpu

MIX4 = (0.05, 0.3, 0.3, 0.2)
CIRCUITS = {
    "sha9": lambda: S.sha_shaped_circuit(9, seed=11, table_bits=2),
    "sha9_tid_var": lambda: S.sha_shaped_circuit(9, seed=11, table_bits=2, table_id_as_variable=True),
    "rec8": lambda: S.recursion_like_circuit(8, seed=2),
    "rec8_p2_op_list": lambda: S.recursion_like_circuit(8, seed=2, poseidon2_as_op_list=True),
    "rec8_p1_kind": lambda: S.recursion_like_circuit(8, seed=2, poseidon1="kind"),
    "rec8_p1_witness": lambda: S.recursion_like_circuit(8, seed=2, poseidon1=8),
    "witness_gates": lambda: S.sha_shaped_circuit(9, seed=5, table_bits=2, gates=S.witness_gates(60, 4, 5), mix=MIX4, num_witness_cols=5),
    "host_gates": lambda: S.sha_shaped_circuit(9, seed=5, table_bits=2, gates=S.host_gates(), mix=MIX4),
}
_cache = {}


def _circuit(name):
    if name not in _cache:
        _cache[name] = CIRCUITS[name]()
    return _cache[name]


def _queries(security, cap, pow_bits, fri_lde, log_n):
    return B.fri_schedule(security, cap, pow_bits, fri_lde.bit_length() - 1, log_n)


def _accepts(c, fri_lde=8, cap=16, security=20, pow_bits=0, **kw):
    """Setup, proof, key both ways, the handle and the words: every combination must say OK with all queries checked."""
    s = E.ProverSetup(ctx(), c, fri_lde, cap, security, pow_bits, **kw)
    try:
        vk = s.verifier()
        buf, on_handle = s.prove_verified(vk)
        on_words = vk.verify(ctx(), buf)
        vk2 = B.Verifier(c, s.cap(), s.config())
        on_created = vk2.verify(ctx(), buf)
        nq = int(buf[9])
        for r in (on_handle, on_words, on_created):
            assert r.stage == B.VERIFY_OK and r.queries_checked == nq, str(r)
        assert on_handle == on_words == on_created
        assert s.verify(buf)
        vk2.close()
        return s, vk, buf
    except Exception:
        s.close()
        raise


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_accepts_what_the_prover_emits_circuits(name):
    s, vk, buf = _accepts(_circuit(name))
    vk.close()
    s.close()


@pytest.mark.parametrize("transcript,hasher", [("poseidon2", None), ("poseidon", None), ("poseidon", "poseidon"), ("blake2s", None),
                                               ("keccak256", None)])
def test_accepts_every_hasher_transcript_pairing(transcript, hasher):
    s, vk, buf = _accepts(_circuit("sha9"), transcript=transcript, tree_hasher=hasher)
    bad = vk.verify(ctx(), bump(buf, Layout(buf).query[1]["setup_path"][0] + 1))
    assert (bad.stage, bad.query, bad.oracle) == (B.VERIFY_MERKLE, 1, 3)
    vk.close()
    s.close()


@pytest.mark.parametrize("pow_bits,runner", [(8, "blake2s"), (8, "keccak256")])
def test_accepts_proof_of_work_with_both_runners(pow_bits, runner):
    s, vk, buf = _accepts(_circuit("sha9"), security=30, pow_bits=pow_bits, pow_runner=runner)
    # the key names the runner: under the other one the proof is refused AT the proof of work, unless its nonce happens to solve
    # that puzzle too (once in 256 at 8 bits) — then the transcript is the same and the proof is valid under both
    from oracle import verifier as OV
    ovk = OV.VerificationKey(_circuit("sha9"), s.cap(), 8, 16)
    other_kind = 2 if runner == "blake2s" else 1
    solves_other = OV.verify(ovk, proof_format.parse(buf, security_level=30), pow_runner=other_kind)
    other = B.Verifier(_circuit("sha9"), s.cap(), dict(s.config(), pow_runner="keccak256" if runner == "blake2s" else "blake2s"))
    r = other.verify(ctx(), buf)
    assert bool(r) == solves_other and (solves_other or r.stage == B.VERIFY_POW), str(r)
    other.close()
    vk.close()
    s.close()


def test_accepts_seven_queries_a_partial_wave():
    s, vk, buf = _accepts(_circuit("sha9"), fri_lde=8, cap=16, security=20)
    assert int(buf[9]) == 7
    vk.close()
    s.close()


def test_accepts_a_hundred_queries_more_than_one_wave_per_oracle():
    s, vk, buf = _accepts(_circuit("rec8"), fri_lde=2, cap=16, security=100)
    assert int(buf[9]) == 100
    L = Layout(buf)
    r = vk.verify(ctx(), bump(buf, L.query[77]["quotient_leaf"][0]))       # a chain of the second wave
    assert (r.stage, r.query, r.oracle, r.queries_checked) == (B.VERIFY_MERKLE, 77, 2, 77)
    vk.close()
    s.close()


def test_accepts_a_zero_depth_fri_path():
    """cap_size = the leaf count of the last FRI layer (2^9 rows x 8 / 2^(3 + 3 + 2) = 16): its openings carry no path, the leaf
    hash is a cap entry."""
    s, vk, buf = _accepts(_circuit("sha9"), fri_lde=8, cap=16, security=20)
    L = Layout(buf)
    assert L.sched == [3, 3, 2] and L.query[0]["fri2_path"][0] == L.query[0]["fri2_path"][1]
    bad = vk.verify(ctx(), bump(buf, L.query[0]["fri2_leaf"][1] - 1))
    assert bad.stage in (B.VERIFY_FRI_MERKLE, B.VERIFY_FRI_VALUE) and (bad.query, bad.oracle) == (0, 2)
    vk.close()
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# edits: the oracle rejects, bj_verify rejects and names the stage
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proven():
    """One proof with lookups, a specialized Boolean gate and proof of work OFF, its keys and the oracle's view of them.  The oracle
    half of every "both reject" below was confirmed without a GPU on the oracle prover's proof of this circuit (the same bytes)."""
    from oracle import verifier as OV
    c = S.sha_shaped_circuit(10, seed=21, table_bits=2, boolean_columns=2)
    s = E.ProverSetup(ctx(), c, 4, 2, 30)       # 15 queries, schedule [3, 3, 3, 1] with paths of 8 + 5 + 2 + 1 digests
    buf, _ = s.prove()
    vk = s.verifier()
    ovk = OV.VerificationKey(c, s.cap(), 4, 2)
    assert vk.verify(ctx(), buf) and OV.verify(ovk, proof_format.parse(buf, security_level=30))
    yield types_ns(c=c, s=s, buf=buf, vk=vk, ovk=ovk, L=Layout(buf), security=30)
    vk.close()
    s.close()


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def _both_reject(pr, words):
    from oracle import verifier as OV
    assert not OV.verify(pr.ovk, proof_format.parse(words, security_level=pr.security))
    r = pr.vk.verify(ctx(), words)
    assert not r
    return r


def test_edited_openings_and_caps(proven):
    pr, L = proven, proven.L
    assert _both_reject(pr, bump(pr.buf, L.ranges["values_at_z"][0] + 34)).stage == B.VERIFY_QUOTIENT
    assert _both_reject(pr, bump(pr.buf, L.ranges["values_at_0"][0] + 3)).stage == B.VERIFY_LOOKUP_SUM
    _both_reject(pr, bump(pr.buf, L.ranges["public_inputs"][0] + 1))
    _both_reject(pr, bump(pr.buf, L.ranges["quotient_cap"][0] + 5))
    _both_reject(pr, bump(pr.buf, L.ranges["fri_caps"][0] + 2))
    assert _both_reject(pr, bump(pr.buf, L.ranges["final_monomials"][0] + 1)).stage == B.VERIFY_FINAL


def test_edited_query_openings(proven):
    pr, L = proven, proven.L
    r = _both_reject(pr, bump(pr.buf, L.query[2]["witness_leaf"][0] + 40))
    assert (r.stage, r.query, r.oracle, r.queries_checked) == (B.VERIFY_MERKLE, 2, 0, 2)
    r = _both_reject(pr, bump(pr.buf, L.query[1]["setup_path"][0] + 6))
    assert (r.stage, r.query, r.oracle) == (B.VERIFY_MERKLE, 1, 3)
    last = L.nq - 1
    assert L.query[last]["fri3_path"][1] > L.query[last]["fri3_path"][0]
    r = _both_reject(pr, bump(pr.buf, L.query[last]["fri3_path"][0] + 2))
    assert (r.stage, r.query, r.oracle) == (B.VERIFY_FRI_MERKLE, last, 3)


def test_edited_fri_leaf_with_its_path_recomputed(proven):
    """The carried slot of query 0's layer-1 leaf changed, the path walked again and the cap entry it ends at replaced: the layer's
    path verifies, the value folded out of layer 0 is no longer in the leaf."""
    pr, L = proven, proven.L
    layer = 1
    words = fri_value_edit(pr.buf, L, layer, query=0)
    r = _both_reject(pr, words)
    assert (r.stage, r.query, r.oracle) == (B.VERIFY_FRI_VALUE, 0, layer)


def test_stored_index_word_and_buffer_shape(proven):
    pr, L = proven, proven.L
    words = np.array(pr.buf, copy=True)
    words[L.index_words[3]] ^= np.uint64(1)
    r = pr.vk.verify(ctx(), words)
    assert (r.stage, r.query) == (B.VERIFY_SHAPE, 3)
    assert pr.vk.verify(ctx(), pr.buf[:-1]).stage == B.VERIFY_SHAPE
    assert pr.vk.verify(ctx(), np.concatenate([pr.buf, np.zeros(1, dtype=np.uint64)])).stage == B.VERIFY_SHAPE
    more = np.array(pr.buf, copy=True)
    more[9] += np.uint64(1)
    assert pr.vk.verify(ctx(), more).stage == B.VERIFY_SHAPE
    huge = np.array(pr.buf, copy=True)
    huge[9] = np.uint64(1 << 62)
    assert pr.vk.verify(ctx(), huge).stage == B.VERIFY_SHAPE
    magic = np.array(pr.buf, copy=True)
    magic[0] += np.uint64(1)
    assert pr.vk.verify(ctx(), magic).stage == B.VERIFY_SHAPE
    assert pr.vk.verify(ctx(), pr.buf[:5]).stage == B.VERIFY_SHAPE
    # the last query removed: refused as a whole proof, accepted as a partial one
    p = proof_format.parse(pr.buf, security_level=pr.security)
    p["queries_per_fri_repetition"] = p["queries_per_fri_repetition"][:-1]
    p["_query_indices"] = p["_query_indices"][:-1]
    short = proof_format.serialize(p, log_n=pr.c.log_n)
    assert pr.vk.verify(ctx(), short).stage == B.VERIFY_SHAPE
    r = pr.vk.verify(ctx(), short, partial=True)
    assert r.stage == B.VERIFY_OK and r.queries_checked == L.nq - 1


def test_edited_keys(proven):
    pr = proven
    cap = pr.s.cap().copy()
    cap[1, 1] = np.uint64((int(cap[1, 1]) + 1) % P)
    other = B.Verifier(pr.c, cap, pr.s.config())
    assert not other.verify(ctx(), pr.buf)
    other.close()
    # the key of the same circuit without the Boolean constraint on its specialized columns
    from era_boojum_amd import gate_program as GP
    c2 = copy.copy(pr.c)
    g = copy.copy(pr.c.specialized_gates[0])
    g.program = GP.GateProgram([(GP.OP_SUB, 0, (0, 0), (0, 0))], [], [(3, 0)], 1)
    c2.specialized_gates = [g]
    lacking = B.Verifier(c2, pr.s.cap(), pr.s.config())
    assert lacking.verify(ctx(), pr.buf).stage == B.VERIFY_QUOTIENT
    lacking.close()


def test_nonce_of_a_proof_of_work():
    from oracle import verifier as OV
    c = _circuit("sha9")
    s = E.ProverSetup(ctx(), c, 8, 16, 30, 8)
    buf, _ = s.prove()
    ovk = OV.VerificationKey(c, s.cap(), 8, 16)
    assert s.verify(buf) and OV.verify(ovk, proof_format.parse(buf, security_level=30))
    for delta in range(1, 4):       # a neighbouring nonce solves an 8-bit puzzle once in 256: take one that does not
        bad = np.array(buf, copy=True)
        bad[18] += np.uint64(delta)
        if not OV.verify(ovk, proof_format.parse(bad, security_level=30)) and s.verify(bad).stage == B.VERIFY_POW:
            break
    else:
        pytest.fail("no neighbouring nonce was refused at the proof of work")
    s.close()


def test_seeded_sweep_of_single_word_edits(proven):
    """300 seeded positions of the body (everything behind header and schedule, index words excluded), each set to value + 1: the
    oracle and bj_verify reject every one, and the draw reaches every field class."""
    from oracle import verifier as OV
    pr, L = proven, proven.L
    positions = sweep_positions(L)
    assert len(positions) == 300 and not set(positions) & set(L.index_words)
    classes = {L.classify(pos) for pos in positions}
    assert set(SWEEP_CLASSES) <= classes, set(SWEEP_CLASSES) - classes
    stages = {}
    for pos in positions:
        words = bump(pr.buf, pos)
        r = pr.vk.verify(ctx(), words)
        assert not r, (pos, L.classify(pos))
        stages[r.stage] = stages.get(r.stage, 0) + 1
        assert not OV.verify(pr.ovk, proof_format.parse(words, security_level=pr.security)), (pos, L.classify(pos))
    print("stages of the 300 edits:", {B.VERIFY_STAGE_NAMES[k]: v for k, v in sorted(stages.items())})


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own proof
# ---------------------------------------------------------------------------------------------------------------------------
def _golden_words(fx, proof=None):
    """The fixture's proof (six of 100 query openings) as BJPF words; the stored index words are the indices the transcript draws
    (the reference's Proof carries none), drawn with the oracle's transcript: independent of the code under test."""
    import oracle as O
    p = proof or golden_proof_dict(fx)
    g = fx["geometry"]
    log_n, log_fri = g["domain_size"].bit_length() - 1, fx["proof_config"]["fri_lde_factor"].bit_length() - 1
    t = O.Transcript()
    t.absorb_cap(np.array(fx["setup_merkle_tree_cap"], dtype=np.uint64))
    t.absorb(p["public_inputs"])
    t.absorb_cap(np.array(p["witness_oracle_cap"], dtype=np.uint64))
    for _ in range(4):
        t.challenge_ext()
    t.absorb_cap(np.array(p["stage_2_oracle_cap"], dtype=np.uint64))
    t.challenge_ext()
    t.absorb_cap(np.array(p["quotient_oracle_cap"], dtype=np.uint64))
    t.challenge_ext()
    for grp in ("values_at_z", "values_at_z_omega", "values_at_0"):
        for v in p[grp]:
            t.absorb(v)
    t.challenge_ext()
    for cap in [p["fri_base_oracle_cap"]] + p["fri_intermediate_oracles_caps"]:
        t.absorb_cap(np.array(cap, dtype=np.uint64))
        t.challenge_ext()
    t.absorb(p["final_fri_monomials"][0])
    t.absorb(p["final_fri_monomials"][1])
    qi = O.QueryIndexer(log_n, log_fri)
    p = dict(p)
    p["_query_indices"] = [qi.next(t) for _ in p["queries_per_fri_repetition"]]
    return proof_format.serialize(p)


def test_the_references_own_proof(fixture_json):
    fx = fixture_json
    assert fx["proof_config"]["pow_bits"] == 0
    vk = B.Verifier(golden_circuit(fx), np.array(fx["setup_merkle_tree_cap"], dtype=np.uint64), golden_config(fx))
    words = _golden_words(fx)
    r = vk.verify(ctx(), words, partial=True)
    assert r.stage == B.VERIFY_OK and r.queries_checked == 6, str(r)
    assert vk.verify(ctx(), words).stage == B.VERIFY_SHAPE              # all 100 queries are required without the flag

    def tampered(edit):
        p = copy.deepcopy(golden_proof_dict(fx))
        edit(p)
        return vk.verify(ctx(), _golden_words(fx, p), partial=True)

    def inc(lst, i, j=None):
        if j is None:
            lst[i] = (lst[i] + 1) % P
        else:
            lst[i][j] = (lst[i][j] + 1) % P
    # the seven tamperings of tests/test_oracle_fixture.py::test_whole_proof_verifier_accepts_the_golden_proof
    assert tampered(lambda p: inc(p["values_at_z"], 200, 0)).stage == B.VERIFY_QUOTIENT
    assert tampered(lambda p: inc(p["values_at_0"], 3, 1)).stage == B.VERIFY_LOOKUP_SUM
    assert not tampered(lambda p: inc(p["public_inputs"], 1))
    r = tampered(lambda p: inc(p["queries_per_fri_repetition"][2]["witness_query"]["leaf_elements"], 40))
    assert (r.stage, r.query, r.oracle) == (B.VERIFY_MERKLE, 2, 0)
    r = tampered(lambda p: inc(p["queries_per_fri_repetition"][4]["fri_queries"][3]["proof"][0], 2))
    assert (r.stage, r.query, r.oracle) == (B.VERIFY_FRI_MERKLE, 4, 3)
    assert not tampered(lambda p: inc(p["final_fri_monomials"][1], 5))
    assert not tampered(lambda p: inc(p["quotient_oracle_cap"][7], 0))
    vk.close()
    lacking = B.Verifier(golden_circuit(fx, with_boolean_gate=False), np.array(fx["setup_merkle_tree_cap"], dtype=np.uint64), golden_config(fx))
    assert lacking.verify(ctx(), words, partial=True).stage == B.VERIFY_QUOTIENT       # the boolean gate matters
    lacking.close()


def test_a_verify_leaves_the_context_as_it_was():
    c = _circuit("sha9")
    s = E.ProverSetup(ctx(), c, 8, 16, 30)
    before, _ = s.prove()
    assert s.verify(before)
    assert not s.verify(bump(before, len(before) - 3))
    after, _ = s.prove()
    assert np.array_equal(before, after)
    s.close()
