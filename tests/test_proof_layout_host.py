"""The layout of a proof (csrc/proof_layout.h: the columns of the four base oracles, the opening order and its named positions, the
opening sets, the header words, the sections of a serialised proof and the words of a query) without a GPU: the header is plain
C++, so one stand-alone program (tests/proof_layout_check.cpp) lays out seven circuit shapes under the address and
undefined-behaviour sanitizers and checks what must hold for any shape.  It also lays out the golden proof's circuit and compares
with counts that come from the reference's proof itself: the lengths of values_at_z and values_at_0 and the four leaf widths of
the fixture's first query, handed over on the command line.  That the prover and the verifier put the same bytes there is what the
proofs of tests/test_gpu_prover.py and tests/test_gpu_verify.py compare."""
import os
import subprocess

from verify_util import golden_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_proof_layouts_hold_their_invariants_and_the_golden_counts_under_the_sanitizers(tmp_path, fixture_json):
    fx = fixture_json
    c = golden_circuit(fx)
    q0 = fx["queries"][0]
    numbers = [c.num_vars, c.num_witness_cols, c.num_constant_cols, c.num_gp_vars, c.lookup_width, c.lookup_reps, c.table_id_col, c.quotient_degree,
               len(fx["values_at_z"]), len(fx["values_at_0"])]
    numbers += [len(q0[k]["leaf_elements"]) for k in ("witness_query", "stage_2_query", "quotient_query", "setup_query")]
    exe = str(tmp_path / "proof_layout_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "proof_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + [str(x) for x in numbers], capture_output=True, text=True)
    assert r.returncode == 0 and "proof layout == expected" in r.stdout, r.stdout + r.stderr
