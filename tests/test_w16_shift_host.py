"""The butterflies by 16th roots of unity of csrc/gl.h on the host.  gl::omega(4) is a power of two (2 has order 192 mod p), so the
DFT-16 inside a radix-16 NTT step multiplies by shifts: mul_pow2_weak<S> for S = 12, 24, .., 84 and the butterflies around it are
__host__ __device__, and one stand-alone program (tests/w16_shift_check.cpp) runs their host side on the vectors of tests/w16_cases.py
under the address and undefined-behaviour sanitizers; its output is compared here with Python integers mod p: every exponent, both
directions (both signs of every power of two), the edge words, words that take every branch of the limb algorithm, random pairs.
The device sequences run the same vectors in tests/test_gpu_w16_butterfly.py."""
import os
import subprocess

import pytest

import w16_cases as C
from era_boojum_amd import build as BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_sixteenth_roots_are_signed_powers_of_two():
    t = [t for t in range(16) if pow(2, 12 * t, C.P) == C.OMEGA16]
    assert len(t) == 1 and t[0] % 2 == 1
    assert pow(2, 96, C.P) == C.P - 1 and pow(C.OMEGA16, 8, C.P) == C.P - 1
    for inverse in (False, True):
        shifts = set()
        for e in range(8):
            w = C.root(e, inverse)
            s = [(S, sign) for S in (0,) + C.SHIFTS for sign in (1, -1) if w == sign * pow(2, S, C.P) % C.P]
            assert len(s) == 1
            shifts.add(s[0][0])
        assert shifts == set((0,) + C.SHIFTS)      # every shift is in use in either direction
    assert pow(C.root(3, False) * C.root(3, True), 1, C.P) == 1


def test_vectors_reach_every_branch():
    words = C.branch_words()
    for S in C.SHIFTS:
        assert {C.branch(v, S) for v in words} >= set(C.BRANCHES[S]), S
    for w in C.EDGE:
        assert (w, w) in C.pairs(0)


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("w16") / "w16_shift_check")
    subprocess.run([BUILD.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "w16_shift_check.cpp"), "-o", exe], check=True)
    ps = C.pairs()
    r = subprocess.run([exe], input="".join("%x %x\n" % p for p in ps), capture_output=True, text=True)
    assert r.returncode == 0 and "== 128-bit arithmetic" in r.stderr, r.stderr[-2000:]
    rows = [[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(ps)
    return ps, rows


def test_butterflies_equal_python_integers(host_output):
    ps, rows = host_output
    for (u, v), row in zip(ps, rows):
        assert len(row) == 2 * 16 + 7
        for d, inverse in enumerate((False, True)):
            for e in range(8):
                assert tuple(row[16 * d + 2 * e:16 * d + 2 * e + 2]) == C.butterfly(u, v, e, inverse), (hex(u), hex(v), e, inverse)


def test_products_by_powers_of_two_equal_python_integers(host_output):
    ps, rows = host_output
    for (u, v), row in zip(ps, rows):
        assert row[32:] == [v * pow(2, S, C.P) % C.P for S in C.SHIFTS], hex(v)
