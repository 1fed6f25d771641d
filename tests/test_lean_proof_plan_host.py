"""Lean proofs (BJ_PROOF_LEAN) without a GPU: the workspace plan of the mode (csrc/workspace_plan.h,
WorkspaceShape::lean_oracles) laid out by a stand-alone program under the address and undefined-behaviour sanitizers
(tests/lean_proof_plan_check.cpp), and the binding's switch, which sets BJ_PROOF_LEAN for the proofs inside it, has the library
read it, and leaves the environment as it found it.  That a lean proof is the resident proof is what tests/test_gpu_lean_proofs.py
shows on the device."""
import os
import subprocess

import pytest

import era_boojum_amd as E
from era_boojum_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_lean_proof_plans_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lean_proof_plan_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "lean_proof_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lean proof plan == expected" in r.stdout, r.stdout + r.stderr


class _Lib:
    """bj_env_reload as a recorder of what the environment held when the library was told to read it."""

    def __init__(self):
        self.seen = []

    def bj_env_reload(self):
        self.seen.append(os.environ.get("BJ_PROOF_LEAN"))


@pytest.mark.parametrize("before", [None, "0", "1", "yes"])
def test_switch_is_read_through_env_reload_and_the_environment_left_as_found(before, monkeypatch):
    if before is None:
        monkeypatch.delenv("BJ_PROOF_LEAN", raising=False)
    else:
        monkeypatch.setenv("BJ_PROOF_LEAN", before)
    lib = _Lib()
    with binding.lean_proofs(lib):
        assert os.environ["BJ_PROOF_LEAN"] == "1"
        with binding.lean_proofs(lib, False):       # resident proofs inside a lean block
            assert os.environ["BJ_PROOF_LEAN"] == "0"
        assert os.environ["BJ_PROOF_LEAN"] == "1"
    assert os.environ.get("BJ_PROOF_LEAN") == before
    assert lib.seen == ["1", "0", "1", before]
    with pytest.raises(RuntimeError):
        with binding.lean_proofs(lib):
            raise RuntimeError("a proof failed")
    assert os.environ.get("BJ_PROOF_LEAN") == before and lib.seen[-2:] == ["1", before]


def test_the_library_reads_the_switch_without_a_device():
    """The real bj_env_reload with the switch set and unset: no device is needed to read the environment, and nothing is left behind."""
    lib = E.load_library()
    before = os.environ.get("BJ_PROOF_LEAN")
    with binding.lean_proofs(lib):
        pass
    assert os.environ.get("BJ_PROOF_LEAN") == before
    header = open(os.path.join(ROOT, "include", "boojum_hip.h")).read()
    assert "BJ_PROOF_LEAN" in header and "proof bytes are identical" in header
    assert 'set("BJ_PROOF_LEAN")' in open(os.path.join(CSRC, "ctx.hip")).read()
