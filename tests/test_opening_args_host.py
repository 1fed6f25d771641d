"""From opening sources to the kernels' column lists (csrc/opening_args.h) without a GPU: the header is plain C++, so one stand-alone
program (tests/opening_args_check.cpp), built host-only under the address and undefined-behaviour sanitizers, compares the
flattening of base-field, F_p^2 and mixed source lists (coefficients (ch0, ch1) and (7 ch1, ch0), C = sum ch_k v_k) with schoolbook
F_p^2 arithmetic on 128-bit integers for canonical and non-canonical words, checks the per-set column ranges of a three-set list, the
block size against callee_words.h, a null column array against null entries in it, that a source without a column is named by source
and set and leaves the list unusable, and that the recombination used after barycentric evaluation inverts the flattening.  What the
kernels compute from these lists is compared with the oracle by tests/test_gpu_openings.py and the proofs of tests/test_gpu_prover.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_opening_arguments_equal_the_definition_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "opening_args_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "opening_args_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "opening arguments == the definition" in r.stdout, r.stdout + r.stderr
