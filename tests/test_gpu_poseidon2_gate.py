"""-m gpu: Poseidon2FlattenedGate<8, 12, 4>, the hand-written evaluator (csrc/gate_poseidon.hip, BJ_GATE_POSEIDON2_FLATTENED: the
walk of csrc/poseidon_gate_terms.h under the canonical-u64 policy) through bj_quotient_gates on arbitrary columns that are no
valid witness, against the same gate as an op list.  The counterpart of the first test of tests/test_gpu_poseidon1_gate.py; whole
proofs with this gate are in tests/test_gpu_gate_program.py, its rare S-box products in tests/test_gpu_poseidon_rare_products.py."""
import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import gate_program as GP, synthetic as S
from gpu_util import DevBuf, ctx, rand_gl

pytestmark = pytest.mark.gpu

P = E.P


@pytest.mark.parametrize("n", [1, 255, 256, 257])   # one lane, a block less one lane, one block, a second block of one lane
def test_hand_written_quotient_equals_the_op_list_word_for_word(n):
    """Random columns with words >= p, a 2-bit selector path whose constants are not 0 or 1, outputs pre-filled with non-zero
    and non-canonical words (the operator overwrites them with the sum of the plain kinds, the Poseidon kernel adds to that): the
    kind and GATE_PROGRAM with the reference's capture give the same words.  The capture is routed to the same kernel by its
    fingerprint, so the sum is also rebuilt in python integers from the interpreter's raw terms (bj_gate_program_eval is never
    routed), which equal the program's python evaluation."""
    path = [False, True]
    rng = np.random.default_rng(7700 + n)
    var = rand_gl(rng, (130, n), noncanonical=True)
    con = rand_gl(rng, (2, n), noncanonical=True)
    con[np.isin(con % np.uint64(P), (0, 1))] = P + 5                # rand_gl plants the word p, a selector constant of 0
    var[5, 0], var[129, n - 1], con[1, 0] = P, 2**64 - 1, P + 2     # words >= p whatever the draw
    assert not np.isin(con % np.uint64(P), (0, 1)).any()
    alphas = rand_gl(rng, (118, 2))
    fill = np.uint64(P) + rng.integers(1, 1 << 32, size=(2, n), dtype=np.uint64) - np.uint64(1)
    assert fill.min() >= P
    prog = GP.poseidon2_flattened_program()
    d_var, d_con = DevBuf(var), DevBuf(con)
    outs = []
    for kind, program in ((S.GATE_POSEIDON2_FLATTENED, None), (S.GATE_PROGRAM, prog)):
        d_out = DevBuf(fill)
        gate = S.GateDesc(kind, "Poseidon2FlattenedGate", 7, 0, 130, 1, 130, 0, 118, True, path=path, program=program)
        ctx().quotient_gates(d_var.ptr, n, 130, d_con.ptr, n, 2, [gate], alphas, n, d_out.ptr, d_out.ptr + 8 * n)
        outs.append(d_out.get((2, n)).copy())
        d_out.free()
    assert np.array_equal(outs[0], outs[1])
    d_terms = DevBuf(nelems=118 * n)
    ctx().gate_program_eval(prog, d_var.ptr, n, d_con.ptr, n, 1, 130, 0, n, d_terms.ptr)
    terms = d_terms.get((118, n))
    for i in range(n):
        t = [int(x) for x in terms[:, i]]
        if i in (0, n - 1):
            assert t == prog.evaluate([int(x) for x in var[:, i]], [])
        sel = ((1 - int(con[0, i])) % P) * (int(con[1, i]) % P) % P
        for k in range(2):
            assert int(outs[0][k, i]) == sel * sum(int(alphas[j, k]) * t[j] for j in range(118)) % P, (i, k)
    for b in (d_var, d_con, d_terms):
        b.free()
