"""From a gate's shape to a kernel's arguments (csrc/gate_launch.h) and the launch descriptors of the term kernels
(csrc/term_io.h) without a GPU: both are host code, so one stand-alone program (tests/gate_launch_check.cpp), built host-only
under the address and undefined-behaviour sanitizers, checks that prog_args puts every field where the op-list kernels read it
(path padded to 8, alpha powers offset by 2 * first_term, null powers kept null, the witness columns and their stride for a program
that reads them and none for one that does not, so that the fused launch takes its entries on a circuit with witness columns), that
gate_windows takes the SHA-256 circuit's three hand-written gates with the window count and first power per kind and refuses every list the windowed
kernel cannot run, that path_bits agrees with GateShape::path, and the arithmetic of Cols::at.  What the kernels compute from these
arguments is compared with the definitions by tests/test_gpu_quotient_terms.py, tests/test_gpu_gate_program.py and the proofs of
tests/test_gpu_prover.py."""
import os
import subprocess

from era_boojum_amd import build as BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_gate_launch_arguments_equal_the_expected_ones_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "gate_launch_check")
    subprocess.run([BUILD.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Xarch_host",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "gate_launch_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gate launch arguments == expected" in r.stdout, r.stdout + r.stderr
