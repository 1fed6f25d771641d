"""-m gpu: PoseidonFlattenedGate<8, 12, 4, PoseidonGoldilocks>, the Poseidon (v1) round-function gate: the hand-written evaluator
(csrc/gate_poseidon.hip, BJ_GATE_POSEIDON_FLATTENED) against the op-list interpreter on arbitrary LDE inputs, and whole proofs of
the recursion-class circuit with the v1 gate — hand-written kind, op list (build-time routed, interpreter), with witness
columns — against each other and against the oracle prover, under the default Poseidon2 pairing and the v1 tree hasher."""
import os
import subprocess
import sys

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import gate_program as GP, proof_format, synthetic as S
from gpu_util import DevBuf, ctx, oracle_threads, rand_gl
from oracle import prover as OP
from oracle import verifier as OV
from test_gpu_prover import _compare

pytestmark = pytest.mark.gpu

P = E.P


def test_hand_written_quotient_equals_the_interpreter_on_random_points():
    """Unsatisfying inputs (random LDE values, not reduced): selector * sum alpha_t * term_t from the kernel equals the same sum
    over the interpreter's raw terms of the reference's capture, and those terms equal the python evaluation, at every point."""
    n, path = 1500, [True, False]
    rng = np.random.default_rng(77)
    var = rand_gl(rng, (130, n), noncanonical=True)
    con = rand_gl(rng, (2, n), noncanonical=True)
    alphas = rand_gl(rng, (118, 2))
    d_var, d_con = DevBuf(var), DevBuf(con)
    d_out = DevBuf(nelems=2 * n)
    gate = S.GateDesc(S.GATE_POSEIDON_FLATTENED, "PoseidonFlattenedGate", 7, 0, 130, 1, 130, 0, 118, True, path=path)
    ctx().quotient_gates(d_var.ptr, n, 130, d_con.ptr, n, 2, [gate], alphas, n, d_out.ptr, d_out.ptr + 8 * n)
    got = d_out.get((2, n))
    prog = GP.poseidon_flattened_program()
    d_terms = DevBuf(nelems=118 * n)
    ctx().gate_program_eval(prog, d_var.ptr, n, d_con.ptr, n, 1, 130, 0, n, d_terms.ptr)
    terms = d_terms.get((118, n))
    for i in range(n):
        t = [int(x) for x in terms[:, i]]
        assert t == prog.evaluate([int(x) for x in var[:, i]], [])
        sel = (int(con[0, i]) % P) * ((1 - int(con[1, i])) % P) % P
        for k in range(2):
            want = sel * sum(int(alphas[j, k]) * t[j] for j in range(118)) % P
            assert int(got[k, i]) == want, (i, k)
    for b in (d_var, d_con, d_out, d_terms):
        b.free()


def test_op_list_forms_give_the_kernels_quotient():
    """bj_quotient_gates with the gate as an op list: the reference's capture (routed to the hand-written kernel by its
    fingerprint) and the compact restatement (compiled at run time) add the same quotient contribution as the kind."""
    n, path = 2048, [False, True]
    rng = np.random.default_rng(78)
    var = rand_gl(rng, (130, n), noncanonical=True)
    con = rand_gl(rng, (2, n), noncanonical=True)
    alphas = rand_gl(rng, (118, 2))
    d_var, d_con, d_out = DevBuf(var), DevBuf(con), DevBuf(nelems=2 * n)
    outs = []
    for kind, prog in ((S.GATE_POSEIDON_FLATTENED, None), (S.GATE_PROGRAM, GP.poseidon_flattened_program()),
                       (S.GATE_PROGRAM, GP.poseidon_flattened_compact_program())):
        gate = S.GateDesc(kind, "PoseidonFlattenedGate", 7, 0, 130, 1, 130, 0, 118, True, path=path, program=prog)
        ctx().quotient_gates(d_var.ptr, n, 130, d_con.ptr, n, 2, [gate], alphas, n, d_out.ptr, d_out.ptr + 8 * n)
        outs.append(d_out.get((2, n)).copy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    for b in (d_var, d_con, d_out):
        b.free()


def _prove(c, fri_lde=2, cap=32, sec=30, **kw):
    s = E.ProverSetup(ctx(), c, fri_lde, cap, sec, **kw)
    buf, _ = s.prove()
    s.close()
    return buf


def test_hand_written_kind_op_list_and_interpreter_give_the_same_proof(tmp_path):
    a = S.recursion_like_circuit(10, seed=9, poseidon1="kind")
    b = S.recursion_like_circuit(10, seed=9, poseidon1="op_list")
    assert a.gates[2].kind == 7 and b.gates[2].kind == 5 and np.array_equal(a.variables, b.variables)
    pa, pb = _prove(a), _prove(b)
    assert np.array_equal(pa, pb)
    out = os.path.join(str(tmp_path), "proof.npy")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import torch; torch.cuda.init();"
            "import era_boojum_amd as E; from era_boojum_amd import synthetic as S;"
            "c = S.recursion_like_circuit(10, seed=9, poseidon1='op_list'); s = E.ProverSetup(E.Context(0), c, 2, 32, 30);"
            "np.save(%r, s.prove()[0])") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           os.path.dirname(os.path.abspath(__file__)), out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BJ_GATE_NO_AOT="1", BJ_GATE_NO_JIT="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out), pa)


@pytest.mark.parametrize("log_n,variant,fri_lde,cap", [(8, "kind", 2, 32), (10, "kind", 8, 16), (12, "kind", 2, 32),
                                                        (9, "op_list", 8, 16), (8, 12, 8, 16)])
def test_hip_proof_equals_oracle_proof(log_n, variant, fri_lde, cap):
    c = S.recursion_like_circuit(log_n, seed=20 + log_n, poseidon1=variant)
    osetup = OP.Setup(c, fri_lde, cap, threads=oracle_threads())
    po = OP.prove(c, osetup, fri_lde, cap, security_level=30, threads=oracle_threads())
    gsetup = E.ProverSetup(ctx(), c, fri_lde, cap, 30)
    assert np.array_equal(gsetup.cap(), osetup.cap)
    buf, _ = gsetup.prove()
    pg = proof_format.parse(buf, security_level=30)
    _compare(pg, po)
    assert OV.verify(OV.VerificationKey(c, gsetup.cap(), fri_lde, cap), pg)
    gsetup.close()


def test_v1_gate_under_the_v1_tree_hasher_and_transcript(monkeypatch):
    import poseidon1_layer as PL
    c = S.recursion_like_circuit(8, seed=31, poseidon1="kind")
    layer = PL.poseidon1_layer()
    monkeypatch.setattr(OP, "hashing_layer", lambda hasher: layer)
    osetup = OP.Setup(c, 8, 16, threads=oracle_threads())
    po = OP.prove(c, osetup, 8, 16, security_level=30, threads=oracle_threads(), transcript_kind=2)
    gsetup = E.ProverSetup(ctx(), c, 8, 16, 30, transcript="poseidon", tree_hasher="poseidon")
    assert np.array_equal(gsetup.cap(), osetup.cap)
    buf, _ = gsetup.prove()
    pg = proof_format.parse(buf, security_level=30)
    _compare(pg, po)
    assert OV.verify(OV.VerificationKey(c, gsetup.cap(), 8, 16), pg, transcript_kind=2)
    gsetup.close()


@pytest.mark.parametrize("variant", ["kind", "op_list"])
def test_unsatisfied_v1_row_is_refused(variant):
    c = S.recursion_like_circuit(9, seed=41, poseidon1=variant)
    g = c.gates[2]
    m = np.ones(c.n, dtype=bool)
    for i, bit in enumerate(g.path):
        m &= c.constants[i] == (1 if bit else 0)
    bad = c.variables.copy()
    row = int(np.flatnonzero(m)[2])
    bad[100, row] = (int(bad[100, row]) + 1) % P           # one partial-round S-box input
    gsetup = E.ProverSetup(ctx(), c, 2, 32, 30)
    with pytest.raises(E.BoojumHipError, match="not satisfied"):
        gsetup.prove(variables=bad)
    gsetup.close()
