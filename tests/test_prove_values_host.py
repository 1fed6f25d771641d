"""bj_prove_values without a GPU.  The footprint a values proof is admitted by (csrc/async_admission.h, WorkspaceShape::n_values):
a stand-alone program (tests/prove_values_admission_check.cpp) under the address and undefined-behaviour sanitizers shows that
with n_values = 0 lane_extras and lane_footprint give the numbers they gave before the field existed, at the shapes of
tests/async_admission_check.cpp, and that with n_values > 0 the witness staging alone moves, by n_values * 8 + n * 4 bytes.  The
entry points are declared in include/boojum_hip_diag.h, exported by the library and present in both bindings generated from it, and
the Python binding and the Rust shim reach them."""
import os
import re
import subprocess

import era_boojum_amd as E
from era_boojum_amd import _abi, _abi_diag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")
NEW = ("bj_prove_values", "bj_prove_values_async", "bj_setup_set_witness_placement")
DOORS = ("bj_witness_gather", "bj_witness_gather_sweep_cells")


def test_values_footprint_moves_the_staging_alone_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "prove_values_admission_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "prove_values_admission_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "prove-values admission == expected" in r.stdout, r.stdout + r.stderr


def test_symbols_are_declared_generated_and_exported():
    """The entry points stand in include/boojum_hip_diag.h, beside the pinned set of boojum_hip.h, within ABI version 6."""
    header = open(os.path.join(ROOT, "include", "boojum_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "boojum_hip_diag.h")).read()
    diag_rs = open(os.path.join(ROOT, "rust", "boojum_hip_diag_sys.rs")).read()
    lib = E.load_library()
    for name in NEW + DOORS:
        assert re.search(r"\b%s\(" % name, diag) and name in _abi_diag.SIGNATURES and re.search(r"pub fn %s\(" % name, diag_rs), name
        assert name not in _abi.SIGNATURES
        assert getattr(lib, name) is not None
    assert "#define BJ_ABI_VERSION 6" in header
    # seven arguments each: context, setup, values, their count, counters, their count, the out pointer
    for name in NEW[:2]:
        assert len(_abi_diag.SIGNATURES[name][1]) == 7
    assert "pub fn bj_prove_values_async(ctx: *mut bj_ctx, setup: *const bj_setup, h_values: *const u64, n_values: usize, " \
           "h_multiplicities: *const u32, n_multiplicities: usize, out: *mut *mut bj_ticket) -> c_int;" in diag_rs


def test_binding_and_rust_shim_reach_the_entry_points():
    for method in ("prove_values", "prove_values_async", "set_witness_placement"):
        assert callable(getattr(E.ProverSetup, method))
    for method in ("witness_gather", "witness_gather_sweep_cells"):
        assert callable(getattr(E.Context, method))
    mount = open(os.path.join(ROOT, "rust", "prove_hip.rs")).read()
    assert '#[path = "prove_values_hip.rs"]' in mount and "pub use prove_values_hip::prove_hip_from_values;" in mount
    src = open(os.path.join(ROOT, "rust", "prove_values_hip.rs")).read()
    m = re.search(r"pub fn prove_hip_from_values<(.*?)\n\}\n", src, re.S)
    assert m, "prove_hip_from_values is missing"
    assert "bj_prove_values(" in m.group(1) and "use super::diag_sys::bj_prove_values;" in src
    assert "unimplemented!" not in src and "todo!" not in src
