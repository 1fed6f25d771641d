"""The test-side hashing layer of the Poseidon (v1) tree hasher (tests/poseidon1_layer.py), checked on the CPU:
  * built around the Poseidon2 permutation it reproduces the oracle's Poseidon2 trees, chunked trees, FRI and whole proof
    byte for byte (so the layer's sponge, tree and FRI plumbing are the oracle's);
  * around the v1 permutation its leaf and node rules are a direct overwrite sponge over oracle.poseidon_permutation;
  * its numpy lane-wise v1 permutation equals the oracle's C one."""
import numpy as np
import pytest

import oracle as O
from era_boojum_amd import synthetic as S
from oracle import prover as OP
from oracle import verifier as OV

import poseidon1_layer as PL

P = O.P


def _states(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2**64 - 1, size=(n, 12), dtype=np.uint64, endpoint=True)
    s[0] = 0
    s[1] = P - 1
    s[2] = 2**64 - 1
    s[3, ::2] = P
    return s


def test_numpy_v1_permutation_equals_the_oracle():
    s = _states(300, 3)
    assert np.array_equal(PL.poseidon1_many_np(s), PL.poseidon1_many_c(s))


def _direct_sponge(els, perm):
    st = [0] * 12
    els = [int(x) % P for x in els]
    for i in range(0, len(els), 8):
        blk = els[i:i + 8]
        st[:8] = blk + [0] * (8 - len(blk))
        st = [int(x) for x in perm(np.array(st, dtype=np.uint64))]
    return st[:4]


@pytest.mark.parametrize("width", [1, 5, 8, 9, 93])
def test_v1_leaf_and_node_rules_are_the_overwrite_sponge(width):
    rng = np.random.default_rng(width)
    layer = PL.poseidon1_layer()
    cols = rng.integers(0, 2**64 - 1, size=(width, 16), dtype=np.uint64, endpoint=True)
    cols[:, 0] = 2**64 - 1
    tree = layer.merkle_construct(cols, 4)
    for i in range(16):
        want = _direct_sponge(cols[:, i], O.poseidon_permutation)
        assert [int(x) for x in tree[i]] == want
        assert [int(x) for x in layer.hash_leaf(cols[:, i])] == want
    for j in range(8):                                      # first node layer: perm(L || R || 0)[0..4]
        st = np.zeros(12, dtype=np.uint64)
        st[:4], st[4:8] = tree[2 * j], tree[2 * j + 1]
        assert np.array_equal(tree[16 + j], O.poseidon_permutation(st)[:4])
        assert np.array_equal(layer.hash_node(tree[2 * j], tree[2 * j + 1]), tree[16 + j])
    assert not np.array_equal(tree, O.merkle_construct(cols, 4))   # not the Poseidon2 tree
    leaf, path = layer.merkle_proof(tree, 16, 4, 5)
    assert layer.merkle_verify(path, layer.merkle_cap(tree, 16, 4), leaf, 5)


@pytest.mark.parametrize("width,leaves,cap", [(5, 64, 16), (9, 32, 1), (16, 16, 4)])
def test_layer_with_poseidon2_equals_the_oracle_trees(width, leaves, cap):
    rng = np.random.default_rng(7 * width)
    layer = PL.poseidon2_layer()
    cols = rng.integers(0, 2**64 - 1, size=(width, leaves), dtype=np.uint64, endpoint=True)
    assert np.array_equal(layer.merkle_construct(cols, cap), O.merkle_construct(cols, cap))
    for log_e in (1, 2, 3):
        srcs = rng.integers(0, 2**64 - 1, size=(2, leaves << log_e), dtype=np.uint64, endpoint=True)
        assert np.array_equal(layer.merkle_construct_chunked(srcs, 1 << log_e, cap), O.merkle_construct_chunked(srcs, 1 << log_e, cap))


def test_layer_with_poseidon2_equals_the_oracle_fri():
    rng = np.random.default_rng(11)
    log_lde, n = 3, 1 << 10
    c0, c1 = rng.integers(0, P, size=n, dtype=np.uint64), rng.integers(0, P, size=n, dtype=np.uint64)
    sched = [3, 3, 1]
    t_o, t_l = O.Transcript(1), O.Transcript(1)
    fo = O.do_fri(c0, c1, log_lde, sched, 4, t_o)
    fl = PL.poseidon2_layer().do_fri(c0, c1, log_lde, sched, 4, t_l)
    for a, b in zip(fo["caps"], fl["caps"]):
        assert np.array_equal(a, b)
    for a, b in zip(fo["trees"], fl["trees"]):
        assert np.array_equal(a, b)
    assert fo["challenges"] == fl["challenges"]
    for a, b in zip(fo["final_monomials"], fl["final_monomials"]):
        assert np.array_equal(a, b)
    assert t_o.challenge() == t_l.challenge()


def _proof_eq(a, b):
    assert set(a) == set(b)
    for k in a:
        assert repr(a[k]) == repr(b[k]), k


def test_layer_with_poseidon2_equals_the_oracle_proof(monkeypatch):
    c = S.sha_shaped_circuit(8, seed=17, table_bits=2)
    osetup = OP.Setup(c, 8, 16, threads=4)
    want = OP.prove(c, osetup, 8, 16, security_level=20, threads=4)
    layer = PL.poseidon2_layer()
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: layer)
    lsetup = OP.Setup(c, 8, 16, threads=4)
    assert np.array_equal(lsetup.tree, osetup.tree)
    got = OP.prove(c, lsetup, 8, 16, security_level=20, threads=4)
    _proof_eq(got, want)
    assert OV.verify(OV.VerificationKey(c, lsetup.cap, 8, 16), got)


def test_v1_layer_proof_is_accepted_by_the_v1_verifier_only(monkeypatch):
    c = S.sha_shaped_circuit(8, seed=18, table_bits=2)
    v1 = PL.poseidon1_layer()
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: v1)
    setup = OP.Setup(c, 8, 16, threads=4)
    proof = OP.prove(c, setup, 8, 16, security_level=20, threads=4, transcript_kind=2)
    vk = OV.VerificationKey(c, setup.cap, 8, 16)
    assert OV.verify(vk, proof, transcript_kind=2)
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: PL.poseidon2_layer())
    assert not OV.verify(vk, proof, transcript_kind=2)
