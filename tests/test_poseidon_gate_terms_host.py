"""The walks of csrc/poseidon_gate_terms.h on the host: the 118 terms of Poseidon2FlattenedGate and PoseidonFlattenedGate under the
F_p^2 policy the verifier runs (and under the host side of the canonical-u64 policy the quotient kernels run, where every
variable is in the base field), against the gates' op lists (gate_program.poseidon2_flattened_program / poseidon_flattened_program)
evaluated over pairs of python integers by oracle/verifier.py::_program_terms_ext, which shares nothing with the product.  The
stand-alone program tests/poseidon_gate_terms_check.cpp is built for the host with the address and undefined-behaviour sanitizers
and reads the draws and the expected terms from a file.  The device compile of the same walks is compared with the interpreter
by tests/test_gpu_poseidon2_gate.py and tests/test_gpu_poseidon1_gate.py."""
import os
import subprocess

import numpy as np
import pytest

from era_boojum_amd import build as BUILD, gate_program as G
from oracle import verifier as OV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")
P = 0xFFFFFFFF00000001
N_REPS, N_VARS, N_TERMS = 64, 130, 118


def _draws(rng):
    """[64][130][2] words: all-zero, all-one, all (p - 1, p - 1), words >= p in both components (the same residues as a random
    repetition, not reduced), one repetition in the base field (c1 = 0, some words written as p + x), the rest random with c1 != 0."""
    v = rng.integers(0, P, size=(N_REPS, N_VARS, 2), dtype=np.uint64)
    v[:, :, 1] = np.maximum(v[:, :, 1], np.uint64(1))
    v[0] = 0
    v[1] = 1
    v[2] = P - 1
    v[3] = rng.integers(P, 1 << 64, size=(N_VARS, 2), dtype=np.uint64)
    v[3, :4] = [[P, 2**64 - 1], [2**64 - 1, P], [P + 1, P], [P, P + 1]]
    v[4, :, 1] = 0
    v[4, ::3, 0] = P + (v[4, ::3, 0] & np.uint64(0xFFFFFFFE))
    v[5, ::2, 1] = P          # c1 == 0 as a non-canonical word: still the base field
    v[5, 1::2, 1] = 0
    return v


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20261)
    out = []
    for prog in (G.poseidon2_flattened_program(), G.poseidon_flattened_program()):
        assert prog.num_terms == N_TERMS
        v = _draws(rng)
        want = np.array([OV._program_terms_ext(prog, [(int(a) % P, int(b) % P) for a, b in rep], (), ()) for rep in v], dtype=np.uint64)
        assert want.shape == (N_REPS, N_TERMS, 2)
        out.append((v, want))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("poseidon_gate_terms") / "poseidon_gate_terms_check")
    subprocess.run([BUILD.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "poseidon_gate_terms_check.cpp"), "-o", path],
                   check=True)
    return path


def _run(exe, cases, path):
    with open(path, "wb") as f:
        for v, want in cases:
            f.write(np.uint64(len(v)).tobytes())
            for rep, terms in zip(v, want):
                f.write(rep.astype("<u8").tobytes() + terms.astype("<u8").tobytes())
    return subprocess.run([exe, path], capture_output=True, text=True)


def test_walks_equal_the_op_lists_over_the_extension_under_the_sanitizers(exe, cases, tmp_path):
    r = _run(exe, cases, str(tmp_path / "cases.bin"))
    # 64 repetitions x 118 terms x 2 gates, two words each, a third (the u64 policy) in the three base-field repetitions
    n_base = 3                                                    # all-zero, c1 = 0 throughout, c1 in {0, p}
    assert [int(np.all(v[:, :, 1] % P == 0, axis=1).sum()) for v, _ in cases] == [n_base, n_base]
    words = 2 * N_TERMS * (2 * N_REPS + n_base)
    assert r.returncode == 0 and "walks == op lists over F_p^2: %d words, %d repetitions" % (words, 2 * n_base) in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("gate,rep,term", [(0, 9, 0), (0, 4, 60), (1, 9, 47), (1, 4, 116)])
def test_a_term_swapped_with_its_neighbour_is_refused(exe, cases, tmp_path, gate, rep, term):
    """An order mistake cannot pass: the expectation with terms `term` and `term + 1` of one repetition exchanged is a mismatch at
    `term` (the program compares, it does not only run)."""
    wrong = [(v, want.copy()) for v, want in cases]
    w = wrong[gate][1]
    assert not np.array_equal(w[rep, term], w[rep, term + 1])
    w[rep, [term, term + 1]] = w[rep, [term + 1, term]]
    r = _run(exe, wrong, str(tmp_path / "wrong.bin"))
    assert r.returncode == 1 and "MISMATCH %s rep %d term %d:" % (("poseidon2", "poseidon1")[gate], rep, term) in r.stdout, r.stdout + r.stderr
