"""The resolved gate list (csrc/gate_list.h: one record per gate with its column starts and its first alpha power, the per-kind
extents, and every refusal about a gate descriptor or the layout of the specialized columns) without a GPU: the header is plain
C++, so one stand-alone program (tests/gate_list_check.cpp) resolves the SHA-256 bench shape, the recursion-class shape and a
circuit with two specialized gates that read constants under the address and undefined-behaviour sanitizers, and compares with
numbers written out by hand; it then provokes each refusal once and checks its code and words.  What the evaluators compute from
these records is compared with the definitions by tests/test_gpu_quotient_terms.py and by the proofs of tests/test_gpu_prover.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_resolved_gate_lists_and_refusals_equal_the_expected_ones_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "gate_list_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "gate_list_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gate list == expected" in r.stdout, r.stdout + r.stderr
