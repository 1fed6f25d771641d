"""The oracle values of the prover (csrc/oracle_value.h) without a GPU: a stand-alone program under the address and
undefined-behaviour sanitizers (tests/oracle_check.cpp) compares what the header answers — the columns of an oracle at a coset, the
sources of an opened polynomial, whether an opening set can be streamed over the FRI domain — with the pointer arithmetic and the
rules the prover and the workspace plan used to spell out at every site, for resident and lean setups and proofs.  That the
proofs are the same bytes is what tests/test_gpu_lean_proofs.py and tests/test_gpu_lean_setup.py show on the device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_oracle_values_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "oracle_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "oracle_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "oracle values == expected" in r.stdout, r.stdout + r.stderr


def test_the_prover_asks_the_values():
    """The residency flags are tested where the values are made and nowhere else in the prover; the plan has no rule of its own."""
    prover = open(os.path.join(CSRC, "prover.hip")).read()
    ctor = prover[prover.index("    Proving(bj_ctx *c"):prover.index("    int reserve_workspace();")]
    rest = prover.replace(ctor, "")
    assert "lean_p" in ctor and "lean_p" not in rest
    assert "S->lean" not in prover and "const u64 *bases[4]" not in prover
    assert "&cols == &sets[0]" not in open(os.path.join(CSRC, "workspace_plan.h")).read()
