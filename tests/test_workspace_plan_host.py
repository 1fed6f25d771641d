"""The workspace plan of a proof (csrc/workspace_plan.h: every buffer a proof takes out of the context's arena, in the order it takes
them, and the reservation as their total) without a GPU: the header is plain C++, so one stand-alone program
(tests/workspace_plan_check.cpp) lays out 120 shapes under the address and undefined-behaviour sanitizers and checks alignment, the
entries of every path, the bench shape's total against the high-water mark DESIGN.md records, and that no plan reserves more than
the hand-written sum it replaces.  That a proof takes exactly its plan is what tests/test_gpu_workspace_plan.py measures."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_workspace_plans_hold_their_invariants_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "workspace_plan_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "workspace_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "workspace plan == expected" in r.stdout, r.stdout + r.stderr
