"""-m gpu: the two shape classes of csrc/proof_layout.h that no other proof of the suite reaches end to end.

Public inputs that share a row: synthetic circuits put every public input on a row of its own, and the golden proof (four inputs
on one row) only goes through the verifier.  Here three inputs, two of them on one row and that row not the first one given, go
through bj_prove, the oracle prover, bj_verify and the oracle verifier.

V <= q (one copy-permutation chunk, no partial products): bj_setup_create and bj_vk_create refuse such a circuit, so no proof of it
exists; the layout of that shape is checked on the host (tests/test_proof_layout_host.py) and the refusal here."""
import copy

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, proof_format, synthetic as S
from gpu_util import ctx
from oracle import prover as OP
from oracle import verifier as OV
from test_gpu_prover import _compare
from verify_util import Layout, bump

pytestmark = pytest.mark.gpu


def test_public_inputs_that_share_a_row_prove_and_verify_like_the_oracle():
    log_n, fri_lde, cap, sec = 9, 4, 4, 20
    c = S.sha_shaped_circuit(log_n, seed=63, table_bits=2, num_gp_vars=24, lookup_width=3, lookup_reps=4, num_public_inputs=0)
    assert c.lookup_reps
    c.public_inputs = [(col, row, int(c.variables[col, row])) for col, row in ((6, 17), (1, 40), (9, 40))]   # the shared row comes second
    osetup = OP.Setup(c, fri_lde, cap, threads=8)
    po = OP.prove(c, osetup, fri_lde, cap, security_level=sec, threads=8)
    s = E.ProverSetup(ctx(), c, fri_lde, cap, sec)
    vk = s.verifier()
    try:
        assert np.array_equal(s.cap(), osetup.cap)
        buf, _ = s.prove()
        pg = proof_format.parse(buf, security_level=sec)
        _compare(pg, po)                                       # the bytes of every field, the oracle's
        ovk = OV.VerificationKey(c, s.cap(), fri_lde, cap)
        assert OV.verify(ovk, pg, verbose=True)
        r = vk.verify(ctx(), buf)
        assert r.stage == B.VERIFY_OK and r.queries_checked == int(buf[9]), str(r)
        # the values on the shared row, altered one at a time.  In the proof's words: the transcript absorbs the public inputs
        # first, so every challenge moves and both verifiers refuse (bj_verify has no stage of its own for a public input: the
        # first check the edit reaches is the quotient identity at z)
        L = Layout(buf)
        for i in (1, 2):
            edited = bump(buf, L.ranges["public_inputs"][0] + i)
            assert not OV.verify(ovk, proof_format.parse(edited, security_level=sec))
            r = vk.verify(ctx(), edited)
            print("public input %d altered: bj_verify stage %d" % (i, r.stage))
            assert not r and r.stage == B.VERIFY_QUOTIENT, str(r)
        # ... and handed to the prover: refused at its public-input check, by the input's own number
        for i in (1, 2):
            vals = [v for (_, _, v) in c.public_inputs]
            vals[i] = (vals[i] + 1) % E.P
            with pytest.raises(E.BoojumHipError, match="public input %d" % i):
                s.prove(public_values=vals)
    finally:
        vk.close()
        s.close()


def test_a_single_copy_permutation_chunk_is_refused_by_setup_and_key():
    """log_n 8, LDE 2, cap 4: 36 variable columns under quotient degree 64 are one chunk."""
    c = S.sha_shaped_circuit(8, seed=64, table_bits=2, num_gp_vars=24, lookup_width=3, lookup_reps=4, num_public_inputs=0)
    ok = E.ProverSetup(ctx(), c, 2, 4, 20)
    cap = ok.cap()
    config = ok.config()
    ok.close()
    one_chunk = copy.copy(c)
    one_chunk.quotient_degree = 64
    assert one_chunk.num_vars <= one_chunk.quotient_degree
    with pytest.raises(E.BoojumHipError, match="single copy-permutation chunk"):
        E.ProverSetup(ctx(), one_chunk, 2, 4, 20)
    with pytest.raises(E.BoojumHipError, match="single copy-permutation chunk"):
        B.Verifier(one_chunk, cap, config)
