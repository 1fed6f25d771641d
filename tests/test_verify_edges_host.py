"""CPU-side checks of the helpers tests/test_gpu_verify_edges.py stands on (tests/verify_util.py): the block-edge circuits are
satisfiable and the oracle proves and verifies them under every tree hasher, the edits of query_edit_batch are proofs the oracle
verifier rejects, and expected_rejection names a stage, a query and an oracle for every word of a query's openings."""
import numpy as np
import pytest

from era_boojum_amd import binding as B, proof_format, synthetic as S
import verify_util as U

LOG_N, FRI_LDE, CAP, SECURITY = 7, 4, 16, 20


def _oracle_proof(c, transcript, hasher, monkeypatch):
    """(proof dict of the oracle prover with its drawn indices, the oracle's key) under a pairing."""
    from oracle import prover as OP, verifier as OV
    kind, layer = U.oracle_layer(transcript, hasher)
    with monkeypatch.context() as m:
        m.setattr(OP, "hashing_layer", lambda _hasher: layer)
        setup = OP.Setup(c, FRI_LDE, CAP, threads=2)
        proof = OP.prove(c, setup, FRI_LDE, CAP, security_level=SECURITY, threads=2, transcript_kind=kind)
    cap = np.asarray(setup.cap)
    proof["_query_indices"] = U.drawn_indices(c, cap, proof, c.log_n, FRI_LDE, transcript, hasher)
    return proof, OV.VerificationKey(c, cap, FRI_LDE, CAP)


@pytest.mark.parametrize("W", U.EDGE_WIDTHS)
def test_edge_width_circuits_prove_and_verify_under_every_tree_hasher(W, monkeypatch):
    c = U.circuit_with_witness_width(W, LOG_N)
    assert S.check_satisfied(c)
    assert U.oracle_widths(c)[0] == W and (W % 8, W % 17) in {(0, 11), (1, 12), (6, 0), (7, 1), (7, 0), (7, 16), (0, 0)}
    for transcript, hasher in U.TREE_HASHER_PAIRINGS:
        proof, ovk = _oracle_proof(c, transcript, hasher, monkeypatch)
        words = proof_format.serialize(proof)
        assert tuple(int(x) for x in words[10:14]) == U.oracle_widths(c), (transcript, hasher)
        assert U.oracle_verify(ovk, proof_format.parse(words, security_level=SECURITY), transcript, hasher, monkeypatch), (transcript, hasher)


def test_the_chosen_widths_put_every_base_oracle_on_a_block_edge():
    """What tests/test_gpu_verify_edges.py asserts again on the proofs' headers: over the seven circuits each of the four base
    oracles has a leaf of a multiple of 8 words, and each but the quotient one of a multiple of 17 and of 16 more than one."""
    widths = [U.oracle_widths(U.circuit_with_witness_width(W, LOG_N)) for W in U.EDGE_WIDTHS]
    for o in range(4):
        assert any(w[o] % 8 == 0 for w in widths), o
    for o in (0, 1, 3):
        assert any(w[o] % 17 == 0 for w in widths) and any(w[o] % 17 == 16 for w in widths), o


@pytest.mark.parametrize("transcript,hasher", [("poseidon2", None), ("blake2s", None)])
def test_query_edits_are_rejected_and_every_word_has_an_expectation(transcript, hasher, monkeypatch, capsys):
    c = U.circuit_with_witness_width(96, LOG_N)
    proof, ovk = _oracle_proof(c, transcript, hasher, monkeypatch)
    buf = proof_format.serialize(proof)
    L = U.Layout(buf)
    n_fri = len(L.sched)
    assert L.nq == 10 and L.sched == [3, 2]
    total = 0
    for q in (0, L.nq // 2, L.nq - 1):
        positions, proofs = U.query_edit_batch(buf, L, q)
        block = sum(L.widths) + 16 * L.depth + sum(b - a for name, (a, b) in L.query[q].items() if name.startswith("fri"))
        assert len(positions) == len(proofs) == block and L.index_words[q] not in positions
        assert positions[0] == L.index_words[q] + 1 and positions[-1] + 1 == (L.index_words[q + 1] if q + 1 < L.nq else len(buf))
        stages_seen = set()
        for pos, words in zip(positions, proofs):
            assert int((words != buf).sum()) == 1 and words[pos] != buf[pos]
            want = U.expected_rejection(L, pos)
            assert want is not None, (pos, L.classify(pos))
            stages, query, oracle = want
            assert len(stages) == 1 and stages <= {B.VERIFY_MERKLE, B.VERIFY_FRI_VALUE, B.VERIFY_FRI_MERKLE}
            assert query == q and 0 <= oracle < 4 + n_fri
            assert oracle < (4 if stages == {B.VERIFY_MERKLE} else n_fri)
            stages_seen |= stages
        assert stages_seen == {B.VERIFY_MERKLE, B.VERIFY_FRI_VALUE, B.VERIFY_FRI_MERKLE}
        # two carried words (c0, c1) per layer, and nothing else, are FRI_VALUE
        value = [pos for pos in positions if U.expected_rejection(L, pos)[0] == {B.VERIFY_FRI_VALUE}]
        assert value == sorted(w for layer in range(n_fri) for w in U.carried_words(L, q, layer))
        total += block
    assert U.expected_rejection(L, L.index_words[3]) is None and U.expected_rejection(L, L.ranges["fri_caps"][0]) is None
    # a seeded sample of 24 edits over the first and the last query: the oracle verifier rejects each, at the check expected_rejection names
    said = {"Merkle path of %s_query does not verify" % name: ({B.VERIFY_MERKLE}, o) for o, name in enumerate(U.BASE_ORACLES)}
    for layer in range(n_fri):
        said["FRI layer %d: carried value is not in the leaf" % layer] = ({B.VERIFY_FRI_VALUE}, layer)
        said["FRI layer %d: Merkle path does not verify" % layer] = ({B.VERIFY_FRI_MERKLE}, layer)
    first, last = U.query_edit_batch(buf, L, 0), U.query_edit_batch(buf, L, L.nq - 1)
    pool = list(zip(first[0] + last[0], first[1] + last[1]))
    rng = np.random.default_rng(20261018)
    for i in rng.choice(len(pool), size=24, replace=False):
        pos, words = pool[int(i)]
        capsys.readouterr()
        assert not U.oracle_verify(ovk, proof_format.parse(words, security_level=SECURITY), transcript, hasher, monkeypatch, verbose=True), (pos, L.classify(pos))
        stages, _, oracle = U.expected_rejection(L, pos)
        assert said[capsys.readouterr().out.strip()[len("verify: "):]] == (stages, oracle), (pos, L.classify(pos))
    assert U.oracle_verify(ovk, proof_format.parse(buf, security_level=SECURITY), transcript, hasher, monkeypatch)


def test_a_recomputed_fri_leaf_keeps_its_path_and_is_rejected_by_the_oracle(monkeypatch):
    """fri_value_edit under the Poseidon2, Blake2s and Keccak tree hashers: the edited layer's path leads to the replaced cap
    entry, every other word is the proof's, and the oracle verifier rejects (the replaced cap entry moves the indices it draws, so
    it stops earlier than the carried value: only bj_verify, which judges again at the stored indices, names that)."""
    c = U.circuit_with_witness_width(96, LOG_N)
    for transcript, hasher in (("poseidon2", None), ("blake2s", None), ("keccak256", None)):
        proof, ovk = _oracle_proof(c, transcript, hasher, monkeypatch)
        buf = proof_format.serialize(proof)
        L = U.Layout(buf)
        _, H = U.oracle_layer(transcript, hasher)
        for layer in range(len(L.sched)):
            words = U.fri_value_edit(buf, L, layer, query=1, H=H)
            changed = np.flatnonzero(words != buf)
            slot = U.carried_words(L, 1, layer)[0]
            a, b = L.ranges["fri_caps"]
            assert slot in changed and all(pos == slot or a + layer * 4 * L.cap <= pos < a + (layer + 1) * 4 * L.cap for pos in changed)
            p = proof_format.parse(words, security_level=SECURITY)
            fq = p["queries_per_fri_repetition"][1]["fri_queries"][layer]
            caps = [p["fri_base_oracle_cap"]] + p["fri_intermediate_oracles_caps"]
            tree = (L.indices[1] >> sum(L.sched[:layer])) >> L.sched[layer]
            assert H.merkle_verify(np.array(fq["proof"], dtype=np.uint64).reshape(-1, 4), np.array(caps[layer], dtype=np.uint64),
                                   H.hash_leaf(fq["leaf_elements"]), tree)
            assert not U.oracle_verify(ovk, p, transcript, hasher, monkeypatch)


def test_a_query_moved_to_front_keeps_every_word(monkeypatch):
    c = U.circuit_with_witness_width(96, LOG_N)
    proof, ovk = _oracle_proof(c, "poseidon2", None, monkeypatch)
    buf = proof_format.serialize(proof)
    L = U.Layout(buf)
    moved = U.query_moved_to_front(buf, L, 6)
    LM = U.Layout(moved)
    assert LM.indices[0] == L.indices[6] and LM.indices[6] == L.indices[0] and LM.indices[1:6] == L.indices[1:6]
    a, b = L.index_words[6], L.index_words[7]
    assert np.array_equal(moved[L.index_words[0]:L.index_words[1]], buf[a:b]) and np.array_equal(moved[a:b], buf[L.index_words[0]:L.index_words[1]])
    assert np.array_equal(np.sort(moved), np.sort(buf)) and int((moved != buf).sum()) > 2 * len(L.query[0])
    outside = np.ones(len(buf), dtype=bool)
    outside[L.index_words[0]:L.index_words[1]] = outside[a:b] = False
    assert np.array_equal(moved[outside], buf[outside])
    assert not U.oracle_verify(ovk, proof_format.parse(moved, security_level=SECURITY), "poseidon2", None, monkeypatch)
