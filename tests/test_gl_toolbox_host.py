"""The shared field helpers of csrc/gl.h on the host: gl::Acc160 / Acc160x2 (the 160-bit lazy accumulator and the pair of
them the term kernels keep), inv_chain / e2_inv_chain, mul7, pow7, omega_pow_nat and domain_point are __host__ __device__, so
one stand-alone program (tests/gl_toolbox_check.cpp) compares them with unsigned __int128 arithmetic mod p and with gl::pow /
gl::inv / gl::e2_mul / gl::e2_inv under the address and undefined-behaviour sanitizers, and gl::reduce128 on the edge grid of
tests/field_helper_cases.py.  The device compile of the helpers is compared with Python integers through bj_field_op_batch
(tests/test_gpu_field_helpers.py); the kernels built on them are compared
word for word with independent references by the -m gpu tests (quotient terms, stage ops, openings, gate programs, Poseidon
gates, setup placement, whole proofs)."""
import os
import re
import subprocess

from era_boojum_amd import build as BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_toolbox_equals_128_bit_arithmetic_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "gl_toolbox_check")
    subprocess.run([BUILD.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "gl_toolbox_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gl toolbox == 128-bit arithmetic" in r.stdout, r.stdout + r.stderr


def test_each_helper_is_defined_once():
    """The private copies are gone: no translation unit defines the accumulator, the inversion chain, 7a, x^7 on base-field words
    or the twiddle-table reader next to gl.h's."""
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f != "jit_headers.inc"}
    gone = re.compile(r"Acc160[qgp]|inv_chain[23]|e2_inv_dev|mul7q")
    assert [f for f, t in text.items() if gone.search(t)] == []
    for pattern in (r"struct \w*Acc160\b", r"auto sqn", r"\bu64 pow7\(u64", r"\bu64 mul7\(u64", r"\bu64 omega_pow_nat\("):
        assert [f for f, t in text.items() if re.search(pattern, t)] == ["gl.h"], pattern
    assert len(re.findall(r"struct Acc160\b", text["gl.h"])) == 1 and len(re.findall(r"auto sqn", text["gl.h"])) == 1
