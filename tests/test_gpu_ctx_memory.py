"""-m gpu: the device memory a context keeps between calls (csrc/ctx.hip: twiddle tables, scratch, arena, witness staging) grows,
serves and goes away without changing a result.

Every test runs on a context of its own, so that the buffers start empty and grow inside the test.  Transforms are compared with
the CPU oracle tests/test_gpu_ntt.py uses; proofs with each other, word for word, and their workspace figures with the plan
(tests/test_gpu_workspace_plan.py has the helpers)."""
import numpy as np
import pytest

import oracle as O
import era_boojum_amd as E
from gpu_util import ctx as session_ctx, rand_gl
from test_gpu_workspace_plan import CAP, FRI_LDE, SEC, circuit, plan_summary

pytestmark = pytest.mark.gpu


@pytest.fixture
def own_ctx():
    session_ctx()   # the session's context brings the HIP runtime up in the order torch needs
    c = E.Context(0)
    yield c
    c.close()


def _both_transforms(c, log_n, n_cols, seed):
    """Forward (coset 7) and inverse transforms of n_cols fresh columns on context c against the oracle."""
    a = rand_gl(np.random.default_rng(seed), (n_cols, 1 << log_n), noncanonical=True)
    d_in, d_out = c.upload(a), c.malloc(a.nbytes)
    try:
        c.ntt_forward_batch(d_in, d_out, log_n, n_cols, coset=7)
        assert np.array_equal(c.d2h(d_out, a.shape), O.fft_batch(a, 7))
        c.intt_batch(d_in, d_out, log_n, n_cols)
        got = c.d2h(d_out, a.shape)
        assert np.array_equal(got, O.ifft_batch(a, 1))
        return got
    finally:
        c.free(d_in)
        c.free(d_out)


def test_twiddle_tables_grow_serve_a_prefix_and_survive_a_release(own_ctx):
    """2^4, then 2^10 (both tables grow and are refilled), then 2^4 again (the larger tables serve it as a prefix); then the
    workspace is released (the tables stay, the scratch of the inverse transform goes) and 2^4 gives the same values once more."""
    first = _both_transforms(own_ctx, 4, 3, 41)
    _both_transforms(own_ctx, 10, 3, 42)
    assert np.array_equal(_both_transforms(own_ctx, 4, 3, 41), first)
    own_ctx.release_workspace()
    assert np.array_equal(_both_transforms(own_ctx, 4, 3, 41), first)


def test_scratch_grows_between_in_place_calls_and_copies_back_strided(own_ctx):
    """bj_intt_batch in place goes through the scratch: 3 columns of 2^4, then 5 of 2^8 (the scratch grows).  bj_bitreverse_batch in
    place with a column stride above the length copies out of the scratch column by column (the 2-D copy): the gaps stay."""
    c = own_ctx
    for log_n, n_cols, seed in ((4, 3, 51), (8, 5, 52)):
        a = rand_gl(np.random.default_rng(seed), (n_cols, 1 << log_n), noncanonical=True)
        d = c.upload(a)
        c.intt_batch(d, d, log_n, n_cols)
        got = c.d2h(d, a.shape)
        c.free(d)
        assert np.array_equal(got, O.ifft_batch(a, 1))
    log_n, n_cols, stride = 5, 3, (1 << 5) + 8
    buf = rand_gl(np.random.default_rng(53), (n_cols, stride))
    d = c.upload(buf)
    c.bitreverse_batch(d, d, log_n, n_cols, col_stride=stride)
    got = c.d2h(d, buf.shape)
    c.free(d)
    assert np.array_equal(got[:, :1 << log_n], np.stack([O.bitreverse(np.ascontiguousarray(col[:1 << log_n])) for col in buf]))
    assert np.array_equal(got[:, 1 << log_n:], buf[:, 1 << log_n:])


def test_a_proof_after_a_release_is_the_same_proof_in_the_same_workspace(own_ctx):
    """The smallest circuit of tests/test_gpu_workspace_plan.py from a host witness, so that arena, staging and scratch are all in
    use: proved, the workspace released, proved again.  The same words, and both times the reservation is the plan's total, the
    proof stays inside it and needs no overflow slab."""
    case, c = "recursion_2p10_host_absorbing", circuit("rec10")
    # the powers of the quotient challenge, as the prover counts them: lookup sums, specialized and general gate terms, L_1, chunks
    alpha_terms = ((c.lookup_reps + 1 if c.lookup_reps else 0) + sum(g.reps * g.num_terms for g in list(c.specialized_gates) + list(c.gates))
                   + 1 + -(-c.num_vars // c.quotient_degree))
    total_words = plan_summary(case, alpha_terms)[0]
    setup = E.ProverSetup(own_ctx, c, FRI_LDE, CAP, SEC)
    try:
        proofs = []
        for _ in range(2):
            buf, _ms = setup.prove()
            ws = dict(setup.last_workspace)
            print(ws, "plan total", 8 * total_words)
            assert ws["reserved_bytes"] == 8 * total_words
            assert ws["high_water_bytes"] <= ws["reserved_bytes"] and ws["overflow_slabs"] == 0
            proofs.append(np.array(buf, copy=True))
            own_ctx.release_workspace()
        assert np.array_equal(proofs[0], proofs[1])
    finally:
        setup.close()
