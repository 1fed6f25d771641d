"""bj_verify / bj_verify_batch, the direction the other verifier tests only sample: EVERY word of a query's openings is bound, for
every tree hasher; leaf widths on the block edges of each leaf function (csrc/verify_open.h: the Blake2sTree and KeccakTree policies,
the two sponge instantiations); the carried-value status of deep_fri_status (csrc/verifier.hip) at every FRI layer; every word of
the final monomials.  What each edit must be rejected as comes from the field class of the word and the order the header
documents (verify_util.expected_rejection), never from the code under test; every proof a test left untouched must be
BJ_VERIFY_OK.  tests/test_verify_edges_host.py checks the helpers without a GPU.

Shapes: 2^7 rows with FRI rate 4 — cap 4, security 20 for the sweeps (base paths of 7 digests, schedule [3, 3, 1] whose last
layer has a zero-depth path, 10 queries), cap 16 for the block-edge widths (paths of 5, schedule [3, 2], 10 queries) — and the 2^10
`proven` fixture of tests/test_gpu_verify.py (schedule [3, 3, 3, 1], 15 queries): every fold width k = 1, 2, 3 occurs, and no
query count is a multiple of the wave."""
import time

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, proof_format, synthetic as S
from gpu_util import ctx
from verify_util import (EDGE_WIDTHS, PAIRINGS, TREE_HASHER_PAIRINGS, Layout, bump, circuit_with_witness_width,
                         expected_rejection, fri_value_edit, oracle_layer, oracle_verify, query_edit_batch, query_moved_to_front)
from test_gpu_verify import proven  # noqa: F401  (the module-scoped fixture of the single-proof tests)

pytestmark = pytest.mark.gpu

LOG_N, FRI_LDE, SECURITY = 7, 4, 20
SWEEP_CAP, SWEEP_SCHEDULE = 4, [3, 3, 1]
WIDTH_CAP, WIDTH_SCHEDULE = 16, [3, 2]
_circuits = {}


def _sweep_circuit():
    if "sweep" not in _circuits:
        _circuits["sweep"] = S.sha_shaped_circuit(LOG_N, seed=41, table_bits=1)
    return _circuits["sweep"]


def _report(r):
    return (r.stage, r.query, r.oracle, r.queries_checked)


def _assert_shape(L, schedule):
    """What the issue asks of every case: base paths of at least two digests, the schedule this case stands for (together they
    hold k = 1, 2, 3), and a last wave that is partial."""
    assert L.depth >= 2 and L.sched == schedule and L.nq % 64 != 0, (L.depth, L.sched, L.nq)
    assert {k for sched in (SWEEP_SCHEDULE, WIDTH_SCHEDULE) for k in sched} == {1, 2, 3}


def _oracle_key(c, s, cap):
    from oracle import verifier as OV
    return OV.VerificationKey(c, s.cap(), FRI_LDE, cap)


# ---------------------------------------------------------------------------------------------------------------------------
# a. every word of a query, for every hasher
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript,hasher", PAIRINGS)
def test_every_word_of_the_first_and_the_last_query_is_bound(transcript, hasher, monkeypatch):
    """One proof per pairing; for query 0 and for query nq - 1 (the last lane of a partial wave, the last chain of its record) one
    bj_verify_batch over a `value + 1` copy per word of the query's block — 438 words: four leaves of 93 + 64 + 8 + 105 words,
    four paths of 7 digests, FRI leaves of 16 + 16 + 4 words with paths of 4 + 1 + 0 digests — with the untouched proof first, in
    the middle and last.  No edit is accepted, every report is the one expected_rejection derives from the word's field class, and
    on 16 seeded positions bj_verify alone gives the same report and the oracle verifier rejects under the same transcript and
    tree hasher.  The host half of the 441 proofs of one call (transcript replay and the identity at z, on the library's
    threads) is printed with the kernels' times: measured on an MI355X host, 2 ms (Blake2s, Keccak) to 43 ms (the Poseidon
    transcripts) per call, so both queries are swept for all five pairings."""
    c = _sweep_circuit()
    s = E.ProverSetup(ctx(), c, FRI_LDE, SWEEP_CAP, SECURITY, transcript=transcript, tree_hasher=hasher)
    vk = s.verifier()
    try:
        buf, _ = s.prove()
        L = Layout(buf)
        _assert_shape(L, SWEEP_SCHEDULE)
        assert L.query[0]["fri2_path"][0] == L.query[0]["fri2_path"][1]          # the zero-depth path of the last layer
        judged, pool = 0, []
        for q in (0, L.nq - 1):
            positions, proofs = query_edit_batch(buf, L, q)
            mid = len(proofs) // 2
            t0 = time.perf_counter()
            got = vk.verify_batch(ctx(), [buf] + proofs[:mid] + [buf] + proofs[mid:] + [buf])
            wall = time.perf_counter() - t0
            print("%s/%s query %d: %d proofs in %.0f ms; host %.1f ms, upload %.2f ms, openings %.2f ms, DEEP + FRI %.2f ms"
                  % ((transcript, hasher, q, len(got), 1e3 * wall) + vk.batch_ms(ctx())))
            for r in (got[0], got[mid + 1], got[-1]):
                assert _report(r) == (B.VERIFY_OK, 0, 0, L.nq), str(r)
            edited = got[1:mid + 1] + got[mid + 2:-1]
            assert len(edited) == len(positions)
            accepted = [(pos, L.classify(pos)) for pos, r in zip(positions, edited) if r.stage == B.VERIFY_OK]
            assert not accepted, "ACCEPTED edits of query %d: %s" % (q, accepted)
            wrong = []
            for pos, r in zip(positions, edited):
                stages, query, oracle = expected_rejection(L, pos)
                if r.stage not in stages or (r.query, r.oracle, r.queries_checked) != (query, oracle, query):
                    wrong.append((pos, L.classify(pos), _report(r), (sorted(stages), query, oracle)))
            assert not wrong, "query %d, (position, class, report, expected): %s" % (q, wrong[:8])
            judged += len(edited)
            pool += list(zip(positions, proofs, edited))
        print("%s/%s: %d edited proofs judged, none accepted" % (transcript, hasher, judged))
        ovk = _oracle_key(c, s, SWEEP_CAP)
        assert oracle_verify(ovk, proof_format.parse(buf, security_level=SECURITY), transcript, hasher, monkeypatch)
        rng = np.random.default_rng(20261018)
        for i in rng.choice(len(pool), size=16, replace=False):
            pos, words, in_batch = pool[int(i)]
            assert vk.verify(ctx(), words) == in_batch, (pos, L.classify(pos))
            assert not oracle_verify(ovk, proof_format.parse(words, security_level=SECURITY), transcript, hasher, monkeypatch), (pos, L.classify(pos))
    finally:
        vk.close()
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# b. block-edge leaf widths, for every tree hasher
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transcript,hasher", TREE_HASHER_PAIRINGS)
def test_leaf_widths_on_the_block_edges(transcript, hasher, monkeypatch):
    """Witness leaves on the edges of the 8-word block of Blake2s and the sponges and of the 17-word rate of Keccak
    (verify_util.circuit_with_witness_width; the generator reaches all seven, none is replaced):

        W    mod 8  mod 17                                              stage 2 (mod 8, mod 17)   setup (mod 8, mod 17)
        96     0     11    full last Blake2s block, full sponge block     64 (0, 13)               105 (1, 3)
        97     1     12    one word in the last block                     64 (0, 13)               105 (1, 3)
        102    6      0    Keccak rem == 0                                68 (4, 0)                112 (0, 10)
        103    7      1                                                   68 (4, 0)                113 (1, 11)
        119    7      0                                                   72 (0, 4)                118 (6, 16)
        135    7     16    Keccak rem == 16                               84 (4, 16)               142 (6, 6)
        136    0      0    both edges at once                             80 (0, 12)               136 (0, 0)

    The quotient leaf is 8 words (0, 8) in every case.  So the other three oracles cover: mod 8 in {0, 4} for stage 2, {0, 1, 6}
    for the setup; mod 17 in {0, 4, 12, 13, 16} for stage 2 and {0, 3, 6, 10, 11, 16} for the setup — each of the four oracles
    has a full last 8-word block at least once, and stage 2 and setup see both Keccak edges (rem 0 and rem 16) as well.
    Per width: the proof's header carries the widths, bj_verify and the oracle verifier accept, and one batch of the proof and nine
    edits of query 1's witness leaf — around the first block and the first rate boundary, at the start of the last block and of
    the last rate block, and the last two words — is the proof accepted and every edit BJ_VERIFY_MERKLE of (query 1, oracle 0)."""
    seen = []
    for W in EDGE_WIDTHS:
        c = circuit_with_witness_width(W, LOG_N)
        s = E.ProverSetup(ctx(), c, FRI_LDE, WIDTH_CAP, SECURITY, transcript=transcript, tree_hasher=hasher)
        vk = s.verifier()
        try:
            buf, _ = s.prove()
            L = Layout(buf)
            _assert_shape(L, WIDTH_SCHEDULE)
            assert int(buf[10]) == W == L.widths[0]
            seen.append(L.widths)
            r = vk.verify(ctx(), buf)
            assert _report(r) == (B.VERIFY_OK, 0, 0, L.nq), (W, str(r))
            assert oracle_verify(_oracle_key(c, s, WIDTH_CAP), proof_format.parse(buf, security_level=SECURITY), transcript, hasher, monkeypatch), W
            a, b = L.query[1]["witness_leaf"]
            assert b - a == W
            words = sorted({0, 7, 8, 16, 17, 8 * ((W - 1) // 8), 17 * ((W - 1) // 17), W - 2, W - 1})
            got = vk.verify_batch(ctx(), [buf] + [bump(buf, a + w) for w in words])
            assert _report(got[0]) == (B.VERIFY_OK, 0, 0, L.nq), (W, str(got[0]))
            for w, r in zip(words, got[1:]):
                assert _report(r) == (B.VERIFY_MERKLE, 1, 0, 1), (W, w, str(r))
        finally:
            vk.close()
            s.close()
    print("%s/%s (witness, stage 2, quotient, setup) widths: %s" % (transcript, hasher, seen))
    print("  mod 8: %s\n  mod 17: %s" % ([tuple(w % 8 for w in ws) for ws in seen], [tuple(w % 17 for w in ws) for ws in seen]))
    for o in range(4):
        assert any(ws[o] % 8 == 0 for ws in seen), o


# ---------------------------------------------------------------------------------------------------------------------------
# c. the carried value at every layer
# ---------------------------------------------------------------------------------------------------------------------------
def _carried_value_edits(buf, L, layers, H):
    """[(layer, query, sub, words)]: per layer the edit of verify_util.fri_value_edit for query 0 and for the query whose element
    index `sub` inside the layer's leaf is the largest, so that a high lane is the source of the wave's shuffle.
    A report names the smallest failing query, and the replaced cap entry is absorbed in front of the layer's own fold challenge:
    every query, query 0 first, then fails behind this layer.  So the carried-value status of a later query can never be the
    report of a whole proof.  Its openings are therefore exchanged with query 0's (verify_util.query_moved_to_front) before the
    edit: they are judged in slot 0, at the index stored with them — where bj_verify judges an edit of this kind anyway, the
    changed cap having moved every drawn index."""
    out = []
    for layer in layers:
        shift, mask = sum(L.sched[:layer]), (1 << L.sched[layer]) - 1
        sub = [(idx >> shift) & mask for idx in L.indices]
        high = max(range(L.nq), key=lambda q: (sub[q], -q))
        out.append((layer, 0, sub[0], fri_value_edit(buf, L, layer, 0, H)))
        if high:
            moved = query_moved_to_front(buf, L, high)
            LM = Layout(moved)
            assert LM.indices[0] == L.indices[high] and LM.indices[high] == L.indices[0]
            out.append((layer, high, sub[high], fri_value_edit(moved, LM, layer, 0, H)))
    return out


def _carried_value_rejected_at_its_layer(vk, ovk, buf, L, layers, H, transcript, hasher, monkeypatch, security):
    # only the CARRIED slot is edited: with the cap entry replaced every value folded out of this layer changes (see above), and
    # an edit of any other slot would be rejected as the carried value of the NEXT layer whether or not the verifier looks at
    # that slot — a test that passes for the wrong reason
    cases = _carried_value_edits(buf, L, layers, H)
    print("%s/%s (layer, query, element of the leaf): %s" % (transcript, hasher, [c[:3] for c in cases]))
    assert {layer for layer, _, _, _ in cases} == set(layers) and any(q for _, q, _, _ in cases)
    # the exchange alone: openings that pass at indices that are not the drawn ones are BJ_VERIFY_SHAPE at the first such index
    moved = query_moved_to_front(buf, L, L.nq - 1)
    got = vk.verify_batch(ctx(), [buf] + [words for _, _, _, words in cases] + [buf, moved])
    for r in (got[0], got[-2]):
        assert _report(r) == (B.VERIFY_OK, 0, 0, L.nq), str(r)
    assert _report(got[-1]) == (B.VERIFY_SHAPE, 0, 0, 0) and vk.verify(ctx(), moved) == got[-1], str(got[-1])
    for (layer, q, sub, words), r in zip(cases, got[1:-2]):
        assert _report(r) == (B.VERIFY_FRI_VALUE, 0, layer, 0), (layer, q, sub, str(r))      # slot 0 holds query q's openings
        assert vk.verify(ctx(), words) == r, (layer, q)
        assert not oracle_verify(ovk, proof_format.parse(words, security_level=security), transcript, hasher, monkeypatch), (layer, q)


def test_carried_value_at_every_layer(proven, monkeypatch):  # noqa: F811
    """The schedule [3, 3, 3, 1] of the `proven` fixture: for every layer the carried slot of the layer's leaf changed, its path
    walked again and the cap entry replaced (verify_util.fri_value_edit), for query 0 and for the query with the largest element
    index at that layer (_carried_value_edits), all in one batch.  Each is BJ_VERIFY_FRI_VALUE of (slot 0, layer).  At layer 0
    nothing was folded yet: the mismatch is against the DEEP value h computed from the four opened base leaves; at layer 3 the
    leaf has two elements."""
    import oracle as O
    pr, L = proven, proven.L
    assert L.sched == [3, 3, 3, 1] and L.nq % 64 != 0
    _carried_value_rejected_at_its_layer(pr.vk, pr.ovk, pr.buf, L, range(len(L.sched)), O, "poseidon2", None, monkeypatch, pr.security)


@pytest.mark.parametrize("transcript", ["blake2s", "keccak256"])
def test_carried_value_at_the_first_and_the_last_layer_under_the_byte_hashers(transcript, monkeypatch):
    """The same edit under the Blake2s and Keccak tree hashers (the oracle package's leaf and node functions walk the path), at
    layer 0 — against the DEEP value — and at the last layer of [3, 3, 1], whose path is empty: the leaf hash IS the cap entry."""
    c = _sweep_circuit()
    s = E.ProverSetup(ctx(), c, FRI_LDE, SWEEP_CAP, SECURITY, transcript=transcript)
    vk = s.verifier()
    try:
        buf, _ = s.prove()
        L = Layout(buf)
        _assert_shape(L, SWEEP_SCHEDULE)
        _, H = oracle_layer(transcript, None)
        _carried_value_rejected_at_its_layer(vk, _oracle_key(c, s, SWEEP_CAP), buf, L, (0, len(L.sched) - 1), H, transcript, None, monkeypatch,
                                             SECURITY)
    finally:
        vk.close()
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# d. final monomials
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_word_of_the_final_monomials(proven, monkeypatch):  # noqa: F811
    """Every word of final_monomials edited, one batch: rejected by both verifiers.  The monomials are absorbed before the indices
    are drawn, so the edit moves every index; bj_verify judges again at the stored ones and names a stage up to BJ_VERIFY_FINAL in
    the documented order (the enum's)."""
    pr, L = proven, proven.L
    a, b = L.ranges["final_monomials"]
    assert b - a >= 2
    edits = [bump(pr.buf, pos) for pos in range(a, b)]
    got = pr.vk.verify_batch(ctx(), [pr.buf] + edits)
    assert _report(got[0]) == (B.VERIFY_OK, 0, 0, L.nq)
    for pos, words, r in zip(range(a, b), edits, got[1:]):
        assert B.VERIFY_OK < r.stage <= B.VERIFY_FINAL, (pos, str(r))
        assert pr.vk.verify(ctx(), words) == r, pos
        assert not oracle_verify(pr.ovk, proof_format.parse(words, security_level=pr.security), "poseidon2", None, monkeypatch), pos
