"""The pass plan of the transforms (csrc/ntt_plan.h: which kernels run over which rounds for a 2^log_n-point transform) without a
GPU: the header is plain C++, so one stand-alone program (tests/ntt_plan_check.cpp) checks, under the address and
undefined-behaviour sanitizers, that for every log_n 0..30, aligned or not, two-pass plan on or off, the passes tile the rounds
[0, log_n), obey the rules their launchers rely on, and equal the literal table of plans.  What the kernels compute under these
plans is compared with the oracle by tests/test_gpu_ntt.py (sizes 0..24) and by the proofs of tests/test_gpu_prover.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_every_plan_tiles_its_rounds_and_equals_the_table_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ntt_plan_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "ntt_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ntt plan == table" in r.stdout, r.stdout + r.stderr
