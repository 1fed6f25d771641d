"""Worker of tests/test_gpu_prove_values.py::test_values_admission: one case of the admission of bj_prove_values_async in a fresh
process (BJ_HBM_BUDGET_BYTES is what the first bj_ctx_create reads; the lanes start from nothing).  usage: <case>.  Prints every
figure before it asserts on it; exit status 0 when the case holds.

The footprints are those of tests/async_admission_worker.py (the plan's total through the host helper, the extras restated from
csrc/async_admission.h) plus VB = n_values * 8 + n * 4, the bytes all_values and the u32 counters take in the witness staging of a
values proof: R' = R + VB, Ln' = Ln + VB.  The circuit is that worker's; its placement is the identity over the flattened columns,
so all_values are the variables and n_values = V n.  SLACK as there: 16 MiB a lane for the device allocator's rounding."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import async_admission_worker as W   # noqa: E402

FRI, CAP, SEC, SLACK = W.FRI, W.CAP, W.SEC, W.SLACK


class Run:
    """Context, a setup from the identity placement, the serial values proof under `budget(f)` bytes.  After it the parent holds its
    workspace, the values in its staging included."""

    def __init__(self, log_n, budget):
        import torch
        torch.cuda.init()    # PyTorch-ROCm ships its own HIP runtime: it must be the copy this process loads first
        import era_boojum_amd as E
        self.E, self.c = E, W.circuit(log_n)
        c = self.c
        V, n = c.variables.shape
        self.values = np.ascontiguousarray(c.variables.reshape(-1))
        total = int(np.flatnonzero(c.multiplicities[0])[-1]) + 1
        self.counters = np.ascontiguousarray(c.multiplicities[0, :total].astype(np.uint32))
        self.f = W.footprints(c)
        self.f["VB"] = self.values.size * 8 + n * 4
        print("values bytes %d" % self.f["VB"])
        self.budget = budget(self.f)
        os.environ["BJ_HBM_BUDGET_BYTES"] = str(self.budget)
        self.ctx = E.Context(0)
        self.s = E.ProverSetup.from_placement(self.ctx, c, np.arange(V * n, dtype=np.int64).reshape(V, n), FRI, CAP, SEC)
        self.ref = self.s.prove()[0]                         # bj_prove on the columns
        ws = dict(self.s.last_workspace)
        W.same(self.s.prove_values(self.values, self.counters)[0], self.ref)
        print("budget %d; serial proof %s; serial values proof %s" % (self.budget, ws, self.s.last_workspace))
        assert ws["reserved_bytes"] == self.f["arena_R"] == self.s.last_workspace["reserved_bytes"]   # the arena as before

    def close(self):
        self.s.close()
        self.ctx.close()


def rungs():
    """The admission lines BJ_ASYNC_DEBUG has printed so far are on stderr, which the test prints; the worker reads its own copy."""
    sys.stderr.flush()
    return [l for l in open(LOG).read().splitlines() if "admission:" in l]


def case_values_lane_lean():
    """Budget H' + R' + Ln' + 2 SLACK: one resident lane and one lean lane with their values fit, two resident lanes do not."""
    r = Run(13, lambda f: 2 * (f["R"] + f["VB"]) + f["Ln"] + f["VB"] + 2 * SLACK)
    f, s = r.f, r.s
    assert f["Ln"] + f["VB"] + 2 * SLACK < f["R"] + f["VB"]
    tickets, reserved = [], []
    for _ in range(6):
        if len(tickets) == 2:
            W.same(s.wait(tickets.pop(0))[0], r.ref)
            reserved.append(s.last_workspace["reserved_bytes"])
        tickets.append(s.prove_values_async(r.values, r.counters))
    for t in tickets:
        W.same(s.wait(t)[0], r.ref)                          # the proof bytes are unchanged, lean or not
        reserved.append(s.last_workspace["reserved_bytes"])
    lines = rungs()
    print("reserved %s\n%s" % (reserved, "\n".join(lines)))
    assert set(reserved) <= {f["arena_R"], f["arena_L"]} and reserved.count(f["arena_L"]) >= 1 and reserved.count(f["arena_R"]) >= 1
    first = [re.search(r"admission: (.*?) on lane (\d)( \(lean\))?, reserves (\d+) bytes", l) for l in lines[:2]]
    # lane 0 from nothing: resident, its whole footprint with the values; lane 1 from nothing: the lean rung, the lean footprint with them
    assert first[0].group(1) == "two lanes, resident" and int(first[0].group(4)) == f["R"] + f["VB"], lines[0]
    assert first[1].group(1) == "lane lean" and first[1].group(3) and int(first[1].group(4)) == f["Ln"] + f["VB"], lines[1]
    r.close()


def case_values_refuse():
    """Budget tables + Ln' - 8: eight bytes below the lean footprint with its values on one lane once the parent has released all but
    its tables (enough for a host-witness proof by the same arithmetic): BJ_ERR_OOM from the submission, no ticket."""
    r = Run(12, lambda f: f["tables"] + f["Ln"] + f["VB"] - 8)
    f = r.f
    assert f["VB"] > 8
    try:
        t = r.s.prove_values_async(r.values, r.counters)
    except r.E.BoojumHipError as e:
        msg = str(e)
        print("refused: %s" % msg)
        numbers = [int(x) for x in re.findall(r"\d{4,}", msg)]
        assert "out of device memory" in msg and "BJ_HBM_BUDGET_BYTES" in msg
        assert numbers[0] == f["Ln"] + f["VB"] and numbers[1] == f["Ln"] + f["VB"] - 8, numbers
    else:
        raise AssertionError("a ticket came back: %r" % t)
    W.same(r.s.prove_values(r.values, r.counters)[0], r.ref)
    r.close()


CASES = {"values_lane_lean": case_values_lane_lean, "values_refuse": case_values_refuse}

if __name__ == "__main__":
    # BJ_ASYNC_DEBUG writes to the process's stderr: keep a copy in a file of this run's own and pass everything on at the end
    import tempfile
    LOG = os.path.join(tempfile.mkdtemp(prefix="prove_values_admission_"), "stderr.log")
    saved = os.dup(2)
    fd = os.open(LOG, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    os.dup2(fd, 2)
    try:
        CASES[sys.argv[1]]()
        print("case %s holds" % sys.argv[1])
    finally:
        os.dup2(saved, 2)
        sys.stderr.write(open(LOG).read())
        import shutil
        shutil.rmtree(os.path.dirname(LOG), ignore_errors=True)
