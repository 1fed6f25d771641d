"""The host arithmetic of bj_list_unsatisfied (csrc/list_plan.h: how a capacity falls across the four kinds of a list whose totals
are known, totals[0] as their sum, the rows of a term-evaluation chunk, the entry slots of the device block) without a GPU: the
header is plain C++, so one stand-alone program (tests/list_plan_check.cpp) checks it under the address and undefined-behaviour
sanitizers, the split against a list written out entry by entry.  What the library writes for these answers is what
tests/test_gpu_list_unsatisfied.py compares with the restatement."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_list_plan_holds_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "list_plan_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "list_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "list plan == expected" in r.stdout, r.stdout + r.stderr
