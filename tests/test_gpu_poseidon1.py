"""-m gpu: the Poseidon (v1) tree hasher, BJ_HASHER_POSEIDON = GoldilocksPoseidonSponge<AbsorptionModeOverwrite>
(csrc/poseidon1.hip), against the oracle's v1 permutation and the test-side v1 hashing layer (tests/poseidon1_layer.py, plugged
into the oracle prover and verifier through oracle.prover.hashing_layer):
permutation, every tree entry point, whole proofs (v1 / Poseidon2 transcript, LDE 8 / 16), the drop-in, resident and pipelined
entry points, sharded ranks, the refusals, and the reference's recursive-mode SHA-256 bench configuration."""
import numpy as np
import pytest

import era_boojum_amd as E
import oracle as O
from era_boojum_amd import proof_format, synthetic as S
from gpu_util import ctx, oracle_threads
from oracle import prover as OP
from oracle import verifier as OV
from test_gpu_prover import _compare

import poseidon1_layer as PL

pytestmark = pytest.mark.gpu

P = E.P
HASHER_POSEIDON = 4


def test_permutation_equals_the_oracle():
    rng = np.random.default_rng(1)
    n = 100_003
    st = rng.integers(0, 2**64 - 1, size=(n, 12), dtype=np.uint64, endpoint=True)
    st[0], st[1], st[2] = 0, P - 1, 2**64 - 1
    st[3, ::2], st[4, 1::2] = P, 2**64 - 1
    d = ctx().upload(st)
    ctx().poseidon_permute(d, n)
    got = ctx().d2h(d, (n, 12))
    ctx().free(d)
    assert np.array_equal(got[:64], np.stack([O.poseidon_permutation(x) for x in st[:64]]))
    assert np.array_equal(got, PL.poseidon1_many_np(st))                   # numpy form: checked against C in the CPU tests
    assert not np.array_equal(got[:8], np.stack([O.poseidon2_permutation(x) for x in st[:8]]))


@pytest.mark.parametrize("leaves,cap", [(64, 16), (256, 1), (1024, 4)])
def test_trees_equal_the_v1_layer(leaves, cap):
    layer = PL.poseidon1_layer()
    c = ctx()
    rng = np.random.default_rng(leaves + cap)
    nd = c.merkle_tree_digests(leaves, cap)
    d_tree = c.malloc(32 * nd)
    c.set_tree_hasher(HASHER_POSEIDON)
    try:
        for width in (1, 5, 7, 8, 9, 16, 17, 93):
            cols = rng.integers(0, 2**64 - 1, size=(width, leaves), dtype=np.uint64, endpoint=True)
            want = layer.merkle_construct(cols, cap)
            d_cols = c.upload(cols)
            c.merkle_tree_build(d_cols, leaves, width, leaves, cap, d_tree)
            got = c.d2h(d_tree, (nd, 4))
            assert np.array_equal(got, want), ("strided", width)
            capv = c.merkle_tree_cap(d_tree, leaves, cap)
            assert np.array_equal(capv, layer.merkle_cap(want, leaves, cap))
            c.merkle_tree_build_ptrs([d_cols + 8 * leaves * k for k in reversed(range(width))], leaves, cap, d_tree)
            assert np.array_equal(c.d2h(d_tree, (nd, 4)), layer.merkle_construct(cols[::-1], cap)), ("ptrs", width)
            c.free(d_cols)
            for idx in (0, leaves // 3, leaves - 1):
                leaf, path = layer.merkle_proof(got, leaves, cap, idx)
                assert layer.merkle_verify(path, capv, layer.hash_leaf(cols[:, idx]), idx)
        for log_e in (1, 2, 3):
            srcs = rng.integers(0, 2**64 - 1, size=(2, leaves << log_e), dtype=np.uint64, endpoint=True)
            d_src = c.upload(srcs)
            c.merkle_tree_build_chunked(d_src, d_src + 8 * (leaves << log_e), leaves << log_e, log_e, cap, d_tree)
            assert np.array_equal(c.d2h(d_tree, (nd, 4)), layer.merkle_construct_chunked(srcs, 1 << log_e, cap)), ("chunked", log_e)
            c.free(d_src)
    finally:
        c.set_tree_hasher(1)
        c.free(d_tree)


def _oracle_proof(monkeypatch, c, fri_lde, sec, kind):
    layer = PL.poseidon1_layer()
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: layer)
    osetup = OP.Setup(c, fri_lde, 16, threads=oracle_threads())
    return osetup, OP.prove(c, osetup, fri_lde, 16, security_level=sec, threads=oracle_threads(), transcript_kind=kind)


@pytest.mark.parametrize("log_n,fri_lde,transcript", [(8, 8, "poseidon"), (10, 8, "poseidon"), (8, 8, "poseidon2"), (8, 16, "poseidon")])
def test_proof_equals_the_oracle_with_the_v1_layer(monkeypatch, log_n, fri_lde, transcript):
    kind = {"poseidon2": 1, "poseidon": 2}[transcript]
    c = S.sha_shaped_circuit(log_n, seed=60 + log_n, table_bits=2)
    osetup, po = _oracle_proof(monkeypatch, c, fri_lde, 40, kind)
    gsetup = E.ProverSetup(ctx(), c, fri_lde, 16, 40, transcript=transcript, tree_hasher="poseidon")
    assert np.array_equal(gsetup.cap(), osetup.cap)
    buf, _ = gsetup.prove()
    pg = proof_format.parse(buf, security_level=40)
    _compare(pg, po)
    vk = OV.VerificationKey(c, gsetup.cap(), fri_lde, 16)
    assert OV.verify(vk, pg, verbose=True, transcript_kind=kind)
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: PL.poseidon2_layer())
    assert not OV.verify(vk, pg, transcript_kind=kind)
    gsetup.close()


def test_drop_in_resident_and_pipelined_proofs_are_identical(monkeypatch):
    """bj_prove (host witness: the group-wise absorb-as-you-extend plan), bj_prove_dev and three bj_prove_async tickets."""
    c = S.sha_shaped_circuit(12, seed=71, table_bits=2)
    g = E.ProverSetup(ctx(), c, 8, 16, 40, transcript="poseidon", tree_hasher="poseidon")
    ref, _ = g.prove()
    layer = PL.poseidon1_layer()
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: layer)
    assert OV.verify(OV.VerificationKey(c, g.cap(), 8, 16), proof_format.parse(ref, security_level=40), transcript_kind=2)
    d_v, d_m = ctx().upload(c.variables), ctx().upload(c.multiplicities)
    dev, _ = g.prove_dev(d_v, d_m)
    assert np.array_equal(dev, ref)
    ts = [g.prove_async() for _ in range(3)]
    for t in ts:
        assert np.array_equal(g.wait(t)[0], ref)
    ctx().free(d_v)
    ctx().free(d_m)
    p2 = E.ProverSetup(ctx(), c, 8, 16, 40, transcript="poseidon")     # Poseidon2 trees: another proof
    assert not np.array_equal(p2.prove()[0], ref)
    p2.close()
    g.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_ranks_give_the_single_gpu_bytes(world):
    from era_boojum_amd import scale_replay
    c = S.sha_shaped_circuit(12, seed=73, table_bits=2)
    single = E.ProverSetup(ctx(), c, 8, 16, 30, transcript="poseidon", tree_hasher="poseidon")
    ref, _ = single.prove()
    single.close()
    got = scale_replay.measure(c, world, 8, 16, 30, transcript="poseidon", steps=1, warmup=0, reference_proof=ref,
                               tree_hasher="poseidon")
    assert sorted(got["ranks"]) == list(range(world))
    ctx().release_workspace()


def test_refusals():
    c = S.sha_shaped_circuit(8, seed=75, table_bits=2)
    with pytest.raises(E.BoojumHipError, match="byte tree hasher"):
        E.ProverSetup(ctx(), c, 8, 16, 20, transcript="blake2s", tree_hasher="poseidon")
    with pytest.raises(E.BoojumHipError, match="byte tree hasher"):
        E.ProverSetup(ctx(), c, 8, 16, 20, transcript="poseidon", tree_hasher="blake2s")
    with pytest.raises(E.BoojumHipError):
        ctx().set_tree_hasher(5)
    ctx().set_tree_hasher(HASHER_POSEIDON)
    ctx().set_tree_hasher(1)


def test_recursive_mode_sha256_bench_configuration(monkeypatch):
    """run_sha256_prover_recursive_mode (gadgets/sha256/mod.rs:273-282): GoldilocksPoseidonSponge trees + GoldilocksPoisedonTranscript
    on the real SHA-256 circuit of an 8 KiB message (2^16 rows), LDE 8, cap 16, security 100: the v1 verifier accepts the proof."""
    from era_boojum_amd import sha256_circuit as SHA
    c = SHA.sha256_circuit(SHA.bench_message(8 << 10))
    assert c.log_n == 16
    g = E.ProverSetup(ctx(), c, 8, 16, 100, transcript="poseidon", tree_hasher="poseidon")
    buf, _ = g.prove()
    pg = proof_format.parse(buf, security_level=100)
    layer = PL.poseidon1_layer()
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: layer)
    assert OV.verify(OV.VerificationKey(c, g.cap(), 8, 16), pg, transcript_kind=2)
    g.close()
