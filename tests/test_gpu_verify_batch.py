"""bj_verify_batch (csrc/verifier.hip, csrc/verify_open.h, csrc/verify_batch_plan.h): many proofs of one key in one call.  The
contract is bj_verify on each proof alone — every report of a batch equals it field for field.  bj_verify is the batch path with
one proof, so both sides of that comparison share the kernels and the judge: it pins the contract (a record table of N against N
tables of one), and the absolute expectations beside it carry the weight — every proof a test left untouched must be
BJ_VERIFY_OK with all its queries checked, and every edited one must fail at the (stage, query, oracle) the edit dictates."""
import copy
import dataclasses

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, proof_format, synthetic as S
from gpu_util import ctx
from verify_util import Layout, P, bump, fri_value_edit, golden_circuit, golden_config, golden_proof_dict
from test_gpu_verify import _circuit, _golden_words, proven  # noqa: F401  (proven: the module-scoped fixture of the single-proof tests)

pytestmark = pytest.mark.gpu


def _batch_equals_loop(vk, proofs, untouched=(), partial=False):
    """verify_batch against bj_verify proof by proof (a contract check: both run the same device path, see the module docstring);
    the proofs at the positions `untouched` must be valid, which no shared fault can fake.  Returns the reports."""
    got = vk.verify_batch(ctx(), proofs, partial_queries=partial)
    want = [vk.verify(ctx(), p, partial=partial) for p in proofs]
    assert got == want, "\n".join("%d: batch %s | alone %s" % (i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)
    for i in untouched:
        assert got[i].stage == B.VERIFY_OK and got[i].queries_checked == int(proofs[i][9]), (i, str(got[i]))
    return got


def _witnesses(c, count):
    """`count` distinct satisfying assignments of one circuit: cells of the last row (a Nop row, linked to nothing) rewritten;
    synthetic.check_satisfied confirms each on the CPU."""
    out = [c.variables]
    rng = np.random.default_rng(7)
    for k in range(1, count):
        v = np.array(c.variables, copy=True)
        v[c.num_gp_vars - 1 - k, c.n - 1] = rng.integers(1, P, dtype=np.uint64)
        S.check_satisfied(dataclasses.replace(c, variables=v))
        out.append(v)
    return out


def _distinct_proofs(s, c, count):
    proofs = [s.prove(variables=v)[0] for v in _witnesses(c, count)]
    assert len({p.tobytes() for p in proofs}) == count
    return proofs


# ---------------------------------------------------------------------------------------------------------------------------
# 1. batch equals the loop, all valid
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,count,cfg,nq", [("sha9", 5, dict(fri_lde=8, cap=16, security=20), 7),
                                               ("rec8", 3, dict(fri_lde=2, cap=16, security=100), 100)],
                         ids=["5x7_a_wave_shared_by_proofs", "3x100_a_boundary_inside_a_wave"])
def test_batch_equals_the_loop_all_valid(name, count, cfg, nq):
    from oracle import verifier as OV
    c = _circuit(name)
    s = E.ProverSetup(ctx(), c, cfg["fri_lde"], cfg["cap"], cfg["security"])
    vk = s.verifier()
    try:
        proofs = _distinct_proofs(s, c, count)
        assert all(int(p[9]) == nq for p in proofs)
        _batch_equals_loop(vk, proofs, untouched=range(count))
        ovk = OV.VerificationKey(c, s.cap(), cfg["fri_lde"], cfg["cap"])
        for p in proofs:
            assert OV.verify(ovk, proof_format.parse(p, security_level=cfg["security"]))
    finally:
        vk.close()
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. one bad proof does not move its neighbours
# ---------------------------------------------------------------------------------------------------------------------------
def _fri_value_edit(pr, layer=1, query=0):
    """test_gpu_verify.py::test_edited_fri_leaf_with_its_path_recomputed: the carried slot changed, path and cap entry recomputed."""
    return fri_value_edit(pr.buf, pr.L, layer, query)


def _device_stage_edits(pr):
    L = pr.L
    last = L.nq - 1
    return {
        "merkle_witness": (bump(pr.buf, L.query[2]["witness_leaf"][0] + 40), (B.VERIFY_MERKLE, 2, 0)),
        "merkle_stage_2": (bump(pr.buf, L.query[last]["stage_2_path"][0] + 1), (B.VERIFY_MERKLE, last, 1)),
        "merkle_quotient": (bump(pr.buf, L.query[0]["quotient_leaf"][0]), (B.VERIFY_MERKLE, 0, 2)),
        "merkle_setup": (bump(pr.buf, L.query[1]["setup_path"][0] + 6), (B.VERIFY_MERKLE, 1, 3)),
        "fri_value": (_fri_value_edit(pr), (B.VERIFY_FRI_VALUE, 0, 1)),
        "fri_merkle": (bump(pr.buf, L.query[last]["fri3_path"][0] + 2), (B.VERIFY_FRI_MERKLE, last, 3)),
        "final": (bump(pr.buf, L.ranges["final_monomials"][0] + 1), (B.VERIFY_FINAL, None, None)),
    }


@pytest.mark.parametrize("position", [1, 0, 3], ids=["middle", "first", "last"])
@pytest.mark.parametrize("edit", ["merkle_witness", "merkle_stage_2", "merkle_quotient", "merkle_setup", "fri_value", "fri_merkle", "final"])
def test_one_bad_proof_does_not_move_its_neighbours(proven, edit, position):
    pr = proven
    words, (stage, query, oracle) = _device_stage_edits(pr)[edit]
    proofs = [pr.buf] * 4
    proofs[position] = words
    got = _batch_equals_loop(pr.vk, proofs, untouched=[i for i in range(4) if i != position])
    r = got[position]
    assert r.stage == stage and (query is None or (r.query, r.oracle, r.queries_checked) == (query, oracle, query)), str(r)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. host-stage failures inside a batch
# ---------------------------------------------------------------------------------------------------------------------------
def _host_stage_failures(pr):
    L = pr.L
    magic = np.array(pr.buf, copy=True)
    magic[0] += np.uint64(1)
    return [(pr.buf[:-1], B.VERIFY_SHAPE), (magic, B.VERIFY_SHAPE), (np.concatenate([pr.buf, np.zeros(1, dtype=np.uint64)]), B.VERIFY_SHAPE),
            (None, B.VERIFY_SHAPE), (bump(pr.buf, L.ranges["values_at_0"][0] + 3), B.VERIFY_LOOKUP_SUM),
            (bump(pr.buf, L.ranges["values_at_z"][0] + 34), B.VERIFY_QUOTIENT)]


def test_host_stage_failures_inside_a_batch(proven):
    pr = proven
    bad = _host_stage_failures(pr)
    proofs, valid = [], []
    for words, _ in bad:                      # valid, bad, valid, bad, ..., valid
        valid.append(len(proofs))
        proofs += [pr.buf, words]
    valid.append(len(proofs))
    proofs.append(pr.buf)
    got = pr.vk.verify_batch(ctx(), proofs)
    for k, (words, stage) in enumerate(bad):
        assert got[2 * k + 1].stage == stage, (k, str(got[2 * k + 1]))
        if words is not None:                 # bj_verify refuses a null pointer as an argument: the batch's verdict is the issue's
            assert got[2 * k + 1] == pr.vk.verify(ctx(), words), k
    for i in valid:
        assert got[i] == pr.vk.verify(ctx(), pr.buf) and got[i].stage == B.VERIFY_OK and got[i].queries_checked == pr.L.nq


def test_a_batch_that_ends_on_the_host_launches_nothing(proven):
    pr = proven
    bad = _host_stage_failures(pr)
    assert pr.vk.verify_batch(ctx(), [pr.buf])[0]                     # a batch that launches: the kernel times are not zero
    assert pr.vk.batch_ms(ctx())[2] > 0 and pr.vk.batch_ms(ctx())[3] > 0
    got = pr.vk.verify_batch(ctx(), [w for w, _ in bad])
    assert [r.stage for r in got] == [stage for _, stage in bad]
    host_ms, upload_ms, open_ms, deep_ms = pr.vk.batch_ms(ctx())
    assert host_ms > 0 and (upload_ms, open_ms, deep_ms) == (0.0, 0.0, 0.0)


def test_proof_of_work_failure_inside_a_batch():
    from oracle import verifier as OV
    c = _circuit("sha9")
    s = E.ProverSetup(ctx(), c, 8, 16, 30, 8)
    vk = s.verifier()
    try:
        buf, _ = s.prove()
        ovk = OV.VerificationKey(c, s.cap(), 8, 16)
        for delta in range(1, 4):       # a neighbouring nonce solves an 8-bit puzzle once in 256: take one that does not
            bad = np.array(buf, copy=True)
            bad[18] += np.uint64(delta)
            if not OV.verify(ovk, proof_format.parse(bad, security_level=30)) and vk.verify(ctx(), bad).stage == B.VERIFY_POW:
                break
        else:
            pytest.fail("no neighbouring nonce was refused at the proof of work")
        got = _batch_equals_loop(vk, [buf, bad, buf], untouched=[0, 2])
        assert got[1].stage == B.VERIFY_POW
    finally:
        vk.close()
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the second pass at the stored indices
# ---------------------------------------------------------------------------------------------------------------------------
def test_stored_index_second_pass(proven):
    pr, L = proven, proven.L
    index_word = np.array(pr.buf, copy=True)
    index_word[L.index_words[3]] ^= np.uint64(1)
    final = bump(pr.buf, L.ranges["final_monomials"][0] + 1)
    proofs = [pr.buf, _fri_value_edit(pr), pr.buf, index_word, final, pr.buf]
    got = _batch_equals_loop(pr.vk, proofs, untouched=[0, 2, 5])
    assert (got[1].stage, got[1].query, got[1].oracle) == (B.VERIFY_FRI_VALUE, 0, 1)
    assert (got[3].stage, got[3].query) == (B.VERIFY_SHAPE, 3)
    assert got[4].stage == B.VERIFY_FINAL
    # the second pass alone in its batch, and with nothing but second-pass proofs around it
    _batch_equals_loop(pr.vk, [final])
    _batch_equals_loop(pr.vk, [final, _fri_value_edit(pr), final])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. partial queries
# ---------------------------------------------------------------------------------------------------------------------------
def test_partial_queries_of_different_lengths_in_one_batch(proven):
    pr = proven

    def first(k):
        p = proof_format.parse(pr.buf, security_level=pr.security)
        p["queries_per_fri_repetition"] = p["queries_per_fri_repetition"][:k]
        p["_query_indices"] = p["_query_indices"][:k]
        return proof_format.serialize(p, log_n=pr.c.log_n)
    proofs = [first(1), first(3), pr.buf, first(3), first(1)]
    got = _batch_equals_loop(pr.vk, proofs, untouched=range(5), partial=True)
    assert [r.queries_checked for r in got] == [1, 3, pr.L.nq, 3, 1]
    without = _batch_equals_loop(pr.vk, proofs, untouched=[2])
    assert [r.stage for r in without] == [B.VERIFY_SHAPE, B.VERIFY_SHAPE, B.VERIFY_OK, B.VERIFY_SHAPE, B.VERIFY_SHAPE]
    edited = bump(proofs[1], Layout(proofs[1]).query[2]["setup_leaf"][0])
    got = _batch_equals_loop(pr.vk, [proofs[0], edited, pr.buf], untouched=[0, 2], partial=True)
    assert (got[1].stage, got[1].query, got[1].oracle) == (B.VERIFY_MERKLE, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. every hasher, lookups, public inputs, a zero-depth FRI path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript,hasher", [("poseidon2", None), ("poseidon", None), ("poseidon", "poseidon"), ("blake2s", None),
                                               ("keccak256", None)])
def test_every_hasher_transcript_pairing(transcript, hasher):
    """sha9 has lookups and two public inputs; at fri_lde 8, cap 16 its last FRI layer has a zero-depth path
    (test_gpu_verify.py::test_accepts_a_zero_depth_fri_path)."""
    c = _circuit("sha9")
    assert c.lookup_reps and len(c.public_inputs) == 2
    s = E.ProverSetup(ctx(), c, 8, 16, 20, transcript=transcript, tree_hasher=hasher)
    vk = s.verifier()
    try:
        buf, _ = s.prove()
        L = Layout(buf)
        assert L.sched == [3, 3, 2] and L.query[0]["fri2_path"][0] == L.query[0]["fri2_path"][1]
        got = _batch_equals_loop(vk, [buf, bump(buf, L.query[1]["setup_path"][0] + 1), buf], untouched=[0, 2])
        assert (got[1].stage, got[1].query, got[1].oracle) == (B.VERIFY_MERKLE, 1, 3)
        got = _batch_equals_loop(vk, [buf, buf, bump(buf, L.query[0]["fri2_leaf"][1] - 1)], untouched=[0, 1])
        assert got[2].stage in (B.VERIFY_FRI_MERKLE, B.VERIFY_FRI_VALUE) and (got[2].query, got[2].oracle) == (0, 2)
        got = _batch_equals_loop(vk, [bump(buf, L.ranges["public_inputs"][0] + 1), buf], untouched=[1])
        assert not got[0]
    finally:
        vk.close()
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_edges_empty_single_and_sixty_four_copies(proven):
    pr = proven
    assert pr.vk.verify_batch(ctx(), []) == []
    _batch_equals_loop(pr.vk, [pr.buf], untouched=[0])
    got = pr.vk.verify_batch(ctx(), [pr.buf] * 64)
    alone = pr.vk.verify(ctx(), pr.buf)
    assert alone.stage == B.VERIFY_OK and got == [alone] * 64
    edited = bump(pr.buf, pr.L.query[5]["quotient_path"][0])
    got = pr.vk.verify_batch(ctx(), [pr.buf] * 63 + [edited] + [pr.buf] * 2)
    assert got[:63] + got[64:] == [alone] * 65 and got[63] == pr.vk.verify(ctx(), edited) and got[63].stage == B.VERIFY_MERKLE


def test_thread_count_does_not_change_the_reports(proven, monkeypatch):
    pr = proven
    lib = E.load_library()
    proofs = [pr.buf, bump(pr.buf, pr.L.ranges["values_at_z"][0] + 34), pr.buf, _fri_value_edit(pr)] * 5
    try:
        reports = []
        for threads in ("1", "16", "1000", "0"):       # the last two are clamped to 16 and 1
            monkeypatch.setenv("BJ_VERIFY_THREADS", threads)
            lib.bj_env_reload()
            reports.append(pr.vk.verify_batch(ctx(), proofs))
        assert reports[0] == reports[1] == reports[2] == reports[3]
        assert reports[0][:4] == [pr.vk.verify(ctx(), p) for p in proofs[:4]] and reports[0][0].stage == B.VERIFY_OK
    finally:
        monkeypatch.delenv("BJ_VERIFY_THREADS")
        lib.bj_env_reload()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the context is left as it was
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_batch_leaves_the_context_as_it_was():
    c = _circuit("sha9")
    s = E.ProverSetup(ctx(), c, 8, 16, 30)
    vk = s.verifier()
    try:
        before, _ = s.prove()
        got = vk.verify_batch(ctx(), [before, bump(before, len(before) - 3), before])
        assert got[0] and not got[1] and got[2]
        after, _ = s.prove()
        assert np.array_equal(before, after)
    finally:
        vk.close()
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the reference's own proof
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_references_own_proof_in_a_batch(fixture_json):
    fx = fixture_json
    vk = B.Verifier(golden_circuit(fx), np.array(fx["setup_merkle_tree_cap"], dtype=np.uint64), golden_config(fx))
    try:
        words = _golden_words(fx)
        p = copy.deepcopy(golden_proof_dict(fx))
        leaf = p["queries_per_fri_repetition"][2]["witness_query"]["leaf_elements"]
        leaf[40] = (leaf[40] + 1) % P
        edited = _golden_words(fx, p)
        assert int((edited != words).sum()) == 1
        got = _batch_equals_loop(vk, [words, edited, words], untouched=[], partial=True)
        assert got[0].stage == got[2].stage == B.VERIFY_OK and got[0].queries_checked == got[2].queries_checked == 6
        assert (got[1].stage, got[1].query, got[1].oracle) == (B.VERIFY_MERKLE, 2, 0)
    finally:
        vk.close()
