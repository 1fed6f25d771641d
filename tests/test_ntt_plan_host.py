"""The pass plan of the transforms (csrc/ntt_plan.h: which kernels run over which rounds for a 2^log_n-point transform) without a
GPU: the header is plain C++, so one stand-alone program (tests/ntt_plan_check.cpp) checks, under the address and
undefined-behaviour sanitizers, that for every log_n 0..30, aligned or not, two-pass plan on or off, the passes tile the rounds
[0, log_n), obey the rules their launchers rely on, and equal the literal table of plans.  What the kernels compute under these
plans is compared with the oracle by tests/test_gpu_ntt.py (sizes 0..24) and by the proofs of tests/test_gpu_prover.py.
The same program checks the launch arithmetic that lives beside the plan (columns per workgroup, cosets per ntt_front10 launch) for
the wide-LDE shapes of tests/test_gpu_lde_cosets.py; the second test holds its literal rows to the list the GPU tests are built from."""
import os
import subprocess

import pytest

import lde_coset_shapes as shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ntt_plan") / "ntt_plan_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "ntt_plan_check.cpp"), "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_every_plan_tiles_its_rounds_and_equals_the_table_under_the_sanitizers(check_run):
    r = check_run
    assert r.returncode == 0 and "ntt plan == table" in r.stdout, r.stdout + r.stderr


def test_cols_per_block_and_front10_launches_of_the_wide_lde_shapes(check_run):
    """The program computes every row through ntt_plan.h and fails on a row that differs from its literal claim (exit status, first
    test); here its printed rows are the rows of lde_coset_shapes, no more and no fewer, and every multi-column row really has more
    than one column in some workgroup."""
    lines = check_run.stdout.splitlines()
    assert check_run.returncode == 0, check_run.stdout + check_run.stderr
    assert sorted(l for l in lines if l.startswith("cpb ")) == sorted(shapes.multi_column_line(c) for c in shapes.MULTI_COLUMN)
    assert sorted(l for l in lines if l.startswith("front10 ")) == sorted(shapes.front10_line(c) for c in shapes.FRONT10)
    for c in shapes.MULTI_COLUMN:
        assert c["cpb"] > 1 and c["n_cols"] > 1 and c["groups"] == -(-c["n_cols"] // c["cpb"])
    assert any(len(c["launches"]) == 1 and c["launches"][0][1] < 8 for c in shapes.FRONT10)          # one short launch
    assert sum(len(c["launches"]) == 2 and c["launches"][1][1] < 8 for c in shapes.FRONT10) == 2     # a full launch and a short one
