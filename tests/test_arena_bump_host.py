"""The bump arithmetic of a context's proof workspace (csrc/arena_bump.h: where a request lands, in the arena, the last overflow
slab or a new one, and the high-water mark a proof reports) and the bytes of a twiddle table both ways (twiddle_bytes / twiddle_log,
csrc/async_admission.h) without a GPU: the headers are plain C++, so one stand-alone program (tests/arena_bump_check.cpp) checks
them under the address and undefined-behaviour sanitizers.  The high-water mark is compared, step by step, with a transcription of
the arithmetic arena_alloc had before the header existed.  What the library allocates for these answers is what
tests/test_gpu_ctx_memory.py and tests/test_gpu_workspace_plan.py measure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "era_boojum_amd", "csrc")


def test_arena_bump_and_twiddle_pair_hold_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "arena_bump_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "arena_bump_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "arena bump == expected" in r.stdout, r.stdout + r.stderr
