"""The admission of a bj_prove_async submission (csrc/async_admission.h: which lane takes the proof, with a resident or a lean
workspace, and the bytes that reserves, from the proof's workspace plan, what the lanes and the parent hold and the bytes available)
without a GPU: the header is plain C++, so one stand-alone program (tests/async_admission_check.cpp) walks the ladder under the
address and undefined-behaviour sanitizers for the bench geometry at 2^20 ... 2^24 rows and for the shapes of
tests/test_gpu_async_admission.py: every rung is reached, each threshold is the plan's bytes to the byte, a lane that holds enough
costs nothing, and a submission is refused only below the lean plan on one lane.  What the library does with the decision is what
the GPU test measures."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_admission_ladder_holds_its_thresholds_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "async_admission_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "async_admission_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "async admission == expected" in r.stdout, r.stdout + r.stderr
