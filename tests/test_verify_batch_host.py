"""CPU-side checks of bj_verify_batch: the layout of a batch in device scratch and the chain -> (proof, query) search
(csrc/verify_batch_plan.h) under the address and undefined-behaviour sanitizers in a stand-alone program, the binding's
marshalling (list in, list of reports out), the Rust shim, and the refusal without a context.  bj_verify and bj_verify_batch
both need a live context before they look at a proof (as tests/test_verify_host.py, this file reaches the verifier's host layer
through what needs no device); the prepare / judge split itself is exercised by the GPU tests of both entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import era_boojum_amd as E
from era_boojum_amd import binding as B, build as BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_under_the_sanitizers(tmp_path):
    """N in {1, 2, 63, 64, 65, 1000} proofs with ragged query counts: every offset the plan hands out is used the way the upload
    and the two kernels use it, on a heap block of exactly the planned size (tests/verify_batch_plan_check.cpp)."""
    exe = str(tmp_path / "verify_batch_plan_check")
    subprocess.run([BUILD.HIPCC, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "verify_batch_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 24", r.stdout + r.stderr


class _FakeLib:
    """Stands where libboojum_hip.so stands under Verifier: records what verify_batch hands to bj_verify_batch."""

    def __init__(self):
        self.calls = []

    def bj_verify_batch(self, ctx_h, vk_h, ptrs, sizes, n, flags, reports):
        proofs = []
        for i in range(n):
            assert (ptrs[i] is None) == (sizes[i] == 0)
            proofs.append([] if not sizes[i] else list(np.ctypeslib.as_array(C.cast(ptrs[i], C.POINTER(C.c_uint64)), (sizes[i],))))
        self.calls.append((ctx_h, vk_h, proofs, n, flags))
        for i in range(n):
            reports[i].stage, reports[i].query, reports[i].oracle, reports[i].queries_checked = i % 9, 10 + i, 20 + i, 30 + i
        return 0

    def bj_vk_destroy(self, h):
        pass


class _FakeCtx:
    _h = "ctx"

    def _check(self, rc):
        assert rc == 0


def test_binding_takes_a_list_and_returns_a_list_of_reports():
    lib = _FakeLib()
    vk = B.Verifier(_handle="vk", _lib=lib)
    proofs = [np.arange(5, dtype=np.uint64), None, np.zeros(0, dtype=np.uint64), [7, 8, 9], np.arange(10, dtype=np.uint64)[::2]]
    got = vk.verify_batch(_FakeCtx(), proofs, partial_queries=True)
    assert lib.calls == [("ctx", "vk", [[0, 1, 2, 3, 4], [], [], [7, 8, 9], [0, 2, 4, 6, 8]], 5, B.VERIFY_PARTIAL_QUERIES)]
    assert got == [B.VerifyReport(i % 9, 10 + i, 20 + i, 30 + i) for i in range(5)] and all(isinstance(r, B.VerifyReport) for r in got)
    assert vk.verify_batch(_FakeCtx(), []) == [] and lib.calls[-1][2:] == ([], 0, 0)
    vk._h = None


def test_ctypes_table_and_header_agree_on_the_new_entry_points():
    for name, arity in (("bj_verify_batch", 7), ("bj_verify_batch_ms", 5)):
        assert len(B._SIGNATURES[name][1]) == arity
        assert hasattr(E.load_library(), name)
    header = open(os.path.join(ROOT, "include", "boojum_hip.h")).read()
    assert "#define BJ_VERIFY_BATCH_MAX_PROOFS 65536u" in header
    plan = open(os.path.join(ROOT, "era_boojum_amd", "csrc", "verify_batch_plan.h")).read()
    assert "VERIFY_BATCH_MAX_PROOFS = (size_t)1 << 16" in plan


def test_no_context_is_an_error_not_a_verdict():
    lib = E.load_library()
    reports = (B._VerifyReport * 1)()
    words = np.zeros(4, dtype=np.uint64)
    ptrs = (C.c_void_p * 1)(words.ctypes.data)
    sizes = (C.c_size_t * 1)(4)
    assert lib.bj_verify_batch(None, None, ptrs, sizes, 1, 0, reports) < 0
    assert lib.bj_verify_batch_ms(None, None, None, None, None) < 0


def test_entry_point_counts_agree():
    from test_abi_symbols import header_symbols
    n = len(header_symbols())
    assert n == 132 == len(B._SIGNATURES)
    assert "(%d entry points" % n in open(os.path.join(ROOT, "README.md")).read()
    assert "**%d entry points**" % n in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d functions" % n in open(os.path.join(ROOT, "rust", "boojum_hip_sys.rs")).read()


def test_rust_verify_batch_hip_uses_declared_symbols_only():
    src = open(os.path.join(ROOT, "rust", "prove_hip.rs")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "boojum_hip_sys.rs")).read()
    m = re.search(r"pub fn verify_batch_hip\(ctx: &HipCtx, vk: &HipVk, proofs: &\[&\[u64\]\], partial_queries: bool\) -> Vec<bj_verify_report> \{(.*?)\n\}\n", src, re.S)
    assert m, "verify_batch_hip is missing or has another signature"
    body = m.group(1)
    declared = set(re.findall(r"pub fn (bj_[a-z0-9_]+)", sys_rs))
    used = set(re.findall(r"\b(bj_[a-z0-9_]+)\(", body))
    assert used == {"bj_verify_batch"} and used <= declared
    assert "unimplemented!" not in body and "todo!" not in body
    assert "pub fn bj_verify_batch(ctx: *mut bj_ctx, vk: *const bj_vk, proofs: *const *const u64, n_words: *const usize, n_proofs: usize, flags: c_uint, out: *mut bj_verify_report) -> c_int;" in sys_rs
    assert "pub const BJ_VERIFY_PARTIAL_QUERIES: u32" in sys_rs and "BJ_VERIFY_PARTIAL_QUERIES" in body


def test_thread_switch_is_read_with_the_other_switches_only():
    """BJ_VERIFY_THREADS is read in csrc/ctx.hip::load_env and clamped to 1..16 there; nothing on the call path reads the
    environment or asks the machine for its core count (that 1 and 16 threads report alike: tests/test_gpu_verify_batch.py)."""
    csrc = os.path.join(ROOT, "era_boojum_amd", "csrc")
    readers = [f for f in sorted(os.listdir(csrc)) if "BJ_VERIFY_THREADS\"" in open(os.path.join(csrc, f)).read()]
    assert readers == ["ctx.hip"]
    assert "e.verify_threads = v < 1 ? 1u : v > 16 ? 16u : (unsigned)v;" in open(os.path.join(csrc, "ctx.hip")).read()
    verifier = open(os.path.join(csrc, "verifier.hip")).read()
    assert "hardware_concurrency" not in verifier and "getenv" not in verifier and "bj::env().verify_threads" in verifier
