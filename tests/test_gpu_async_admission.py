"""-m gpu: bj_prove_async admits every submission by the bytes available (csrc/async_admission.h): the device's free
bytes capped by BJ_HBM_BUDGET_BYTES against what the proof's lane wants.  Each case is one fresh process
(tests/async_admission_worker.py, which states the footprints R, Ln, H and the slack and where they come from): the switch is read
by the first bj_ctx_create, and the lanes' arenas must start from nothing.  The worker measures device memory with
torch.cuda.mem_get_info, independently of the library's accounting, and compares every proof with the serial bj_prove's.

  lane_lean        2^13 rows, budget H + R + Ln + 2 slack: six proofs in the documented submit / wait pattern, the second lane lean;
                   the device grows by no more than the budget.  Without admission the lanes take two resident workspaces and pass it.
  one_lane         2^12 rows, budget H + R + slack < H + R + Ln: every proof behind lane 0, a third submission with one in flight.
  release_parent   2^12 rows, budget below the lean lane while the idle parent holds its workspace: it is released, the proof runs
                   lean, a later bj_prove reserves again and gives the same bytes.  (The budget is not below Ln itself: under such
                   a budget nothing fits, which is the next case.)
  refuse           2^10 rows, budget 1 MiB: BJ_ERR_OOM from bj_prove_async with both byte counts, no ticket, bj_prove still works.
  no_budget        2^10 rows: two resident lanes of R bytes each, as before admission (the scratch at its bound, 29 n words more).
  tickets          a second wait, a pointer that was never a ticket, wait and poll after bj_ctx_destroy with a proof nobody waited
                   for: BJ_ERR_INVALID_ARG from the registry, nothing is read through the pointer; Python's wait() raises.

Measured on an MI355X: lane_lean holds 335 566 720 bytes by the library's count under a budget of 371 021 696 and the device is
348 127 232 bytes fuller; one_lane 146 800 640 under 152 987 648; release_parent 41 943 040 under 49 658 368; at 2^10 rows two
resident lanes take 46 137 344 bytes where 2 R = 34 141 696.  These bounds were missed by about 165 MB a lane as long as
lookup_polys_kernel (stage2.hip) kept two small arrays in scratch memory: the runtime reserves a kernel's scratch for every wave
slot of every hardware queue that runs it, and each lane's stream is such a queue.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", ["lane_lean", "one_lane", "release_parent", "refuse", "no_budget", "tickets"])
def test_admission(case):
    env = {k: v for k, v in os.environ.items() if k not in ("BJ_HBM_BUDGET_BYTES", "BJ_PROOF_LEAN", "BJ_ASYNC_MODE")}
    env["BJ_ASYNC_DEBUG"] = "1"   # the rung of every submission, on stderr
    r = subprocess.run([sys.executable, os.path.join(HERE, "async_admission_worker.py"), case], env=env, capture_output=True, text=True,
                       timeout=180)
    print(r.stdout[-6000:])
    print(r.stderr[-6000:])
    assert r.returncode == 0 and "case %s holds" % case in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
