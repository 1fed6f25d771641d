"""Worker of tests/test_gpu_async_admission.py: one case of the admission of bj_prove_async in a fresh process, so that
BJ_HBM_BUDGET_BYTES is what the first bj_ctx_create reads and the lanes' arenas start from nothing.  usage: <case>.  Prints every
figure before it asserts on it; exit status 0 when the case holds.

The footprints come from the library's own parts, none from what the run under test gives:
  arena     the total of the workspace plan (csrc/workspace_plan.h through the host helper) of a bj_prove that absorbs its column
            groups, witness and stage-2 oracles resident (R) or lean (Ln); the first serial bj_prove must report exactly the former;
  extras    csrc/async_admission.h, restated: the witness staging, (V + 1) n words; the scratch bound, every witness or stage-2
            column in one inverse transform; two twiddle tables of n max(fri_lde, q) / 2 words.
H, what the parent holds after a serial bj_prove, is counted as R: the same parts, its scratch being what its transforms asked for,
at most the bound (29 n words less here).  SLACK is a condition, not a measurement: a lane makes eight device allocations (arena,
staging, scratch, three tables, its small constants, its pointer table), each of which may take up to one 2 MiB block of the
device allocator more than the bytes counted for it: 16 MiB a lane.  tests/async_admission_check.cpp checks that it is below the
gap to the next rung at the shapes used here (2 SLACK < R - Ln at 2^13 rows; SLACK < Ln and tables + Ln + SLACK < R at 2^12)."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

FRI, CAP, SEC = 8, 16, 30
SLACK = 16 << 20


def circuit(log_n):
    from era_boojum_amd import synthetic as S
    return S.sha_shaped_circuit(log_n, seed=900 + log_n, table_bits=2)   # the bench geometry: 60 + 8 * 4 columns, width-4 lookups


def plan_bytes(c, lean):
    """Bytes of the workspace plan of a bj_prove (host witness, groups absorbed) of c on one GPU."""
    from era_boojum_amd import binding, build
    lib = C.CDLL(build.build_canon_helper())
    lib.bj_workspace_plan_summary.restype = None
    new_pow, nq, sched, _ = binding.fri_schedule(SEC, CAP, 0, FRI.bit_length() - 1, c.log_n)
    u = lambda xs: (C.c_uint * max(len(xs), 1))(*xs)
    nine = [c.log_n, c.num_vars, c.num_gp_vars, int(getattr(c, "num_witness_cols", 0)), c.num_constant_cols, c.lookup_width, c.lookup_reps,
            c.table_id_col, c.quotient_degree]
    alpha_terms = c.lookup_reps + 1 + sum(g.reps * g.num_terms for g in c.gates) + 1 + -(-c.num_vars // c.quotient_degree)
    out = (C.c_size_t * 4)()
    lib.bj_workspace_plan_summary(u(nine), C.c_uint(FRI), C.c_uint(CAP), C.c_uint(1), C.c_uint(alpha_terms),
                                  u([p[0] for p in c.public_inputs]), u([p[1] for p in c.public_inputs]), C.c_size_t(len(c.public_inputs)),
                                  u([4 if lean else 0, 0, 1, int(new_pow != 0)]), (C.c_uint32 * 32)(*sched), C.c_size_t(len(sched)),
                                  C.c_size_t(nq), out)
    return 8 * int(out[0])


def footprints(c):
    n, V, q = c.n, c.num_vars, c.quotient_degree
    assert c.lookup_reps and not getattr(c, "num_witness_cols", 0) and n * q < 1 << 27
    nW, nS2 = V + 1, 2 * (1 + (-(-V // q) - 1) + c.lookup_reps + 1)
    staging = (V + 1) * n * 8
    scratch = max(max(nW, nS2) * n, 2 * n * q, 2 * n + 2) * 8
    tables = 2 * (n * max(FRI, q) // 2) * 8
    f = dict(arena_R=plan_bytes(c, False), arena_L=plan_bytes(c, True), tables=tables, extras=staging + scratch + tables)
    f["R"], f["Ln"] = f["arena_R"] + f["extras"], f["arena_L"] + f["extras"]
    print("footprints: %s" % f)
    return f


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def same(a, b):
    assert a.shape == b.shape and np.array_equal(a, b), "proofs differ"


class Run:
    """Context, setup and the serial proof of circuit(log_n) under `budget(f)` bytes (None: no switch).  After it the parent holds
    its workspace; free0 is the device's free bytes before that workspace existed (after a warm-up proof that was released)."""

    def __init__(self, log_n, budget):
        import torch
        torch.cuda.init()    # PyTorch-ROCm ships its own HIP runtime: it must be the copy this process loads first
        import era_boojum_amd as E
        self.E, self.c = E, circuit(log_n)
        self.f = footprints(self.c)
        self.budget = budget(self.f) if budget else 0
        if budget:
            os.environ["BJ_HBM_BUDGET_BYTES"] = str(self.budget)
        else:
            os.environ.pop("BJ_HBM_BUDGET_BYTES", None)
        self.ctx = E.Context(0)
        self.s = E.ProverSetup(self.ctx, self.c, FRI, CAP, SEC)
        self.s.prove()                       # warm-up: the kernels are loaded
        self.ctx.release_workspace()
        self.free0 = free_bytes()
        self.ref = self.s.prove()[0]
        ws = dict(self.s.last_workspace)
        self.free1 = free_bytes()
        print("budget %d; serial proof %s; parent's workspace took %d bytes of the device" % (self.budget, ws, self.free0 - self.free1))
        assert ws["reserved_bytes"] == self.f["arena_R"] and ws["overflow_slabs"] == 0

    def async_proofs(self, count, in_flight=2):
        """The documented pattern: `in_flight` tickets out, then one wait per further submission.  Returns the reserved bytes."""
        s, tickets, reserved = self.s, [], []
        for _ in range(count):
            if len(tickets) == in_flight:
                same(s.wait(tickets.pop(0))[0], self.ref)
                reserved.append(s.last_workspace["reserved_bytes"])
            tickets.append(s.prove_async())
        for t in tickets:
            same(s.wait(t)[0], self.ref)
            reserved.append(s.last_workspace["reserved_bytes"])
        grew = self.free0 - free_bytes()
        print("%d async proofs reserved %s; the device holds %d bytes more than before the parent's workspace" % (count, reserved, grew))
        return reserved, grew

    def close(self):
        self.s.close()
        self.ctx.close()


def case_lane_lean():
    """Budget H + R + Ln + 2 SLACK: the second lane fits lean only."""
    r = Run(13, lambda f: f["R"] + f["R"] + f["Ln"] + 2 * SLACK)
    f = r.f
    assert f["Ln"] + 2 * SLACK < f["R"]
    reserved, grew = r.async_proofs(6)
    assert set(reserved) <= {f["arena_R"], f["arena_L"]} and reserved.count(f["arena_L"]) >= 1 and reserved.count(f["arena_R"]) >= 1
    assert grew <= r.budget, "grew %d, budget %d (two resident lanes and the parent: %d)" % (grew, r.budget, 3 * f["R"])
    r.close()


def case_one_lane():
    """Budget H + R + SLACK, below H + R + Ln: every proof behind lane 0, three submissions with one in flight."""
    r = Run(12, lambda f: f["R"] + f["R"] + SLACK)
    f = r.f
    assert SLACK < f["Ln"]
    reserved, grew = r.async_proofs(3, in_flight=3)
    assert reserved == [f["arena_R"]] * 3
    assert grew <= r.budget and grew < 2 * f["R"] + f["arena_L"]
    r.close()


def case_release_parent():
    """Budget tables + Ln + SLACK: below the lean lane while the parent holds its workspace (H + Ln does not fit), enough for it once
    the parent has released it (the tables stay), too little for a resident lane."""
    r = Run(12, lambda f: f["tables"] + f["Ln"] + SLACK)
    f = r.f
    assert r.budget < f["R"] and r.budget < f["R"] - f["tables"] + f["Ln"]
    reserved, grew = r.async_proofs(1)
    assert reserved == [f["arena_L"]]
    assert grew <= r.budget and r.free1 < free_bytes(), "the parent's workspace was not released: %d free before, %d after" % (r.free1, free_bytes())
    same(r.s.prove()[0], r.ref)            # the parent reserves again
    assert r.s.last_workspace["reserved_bytes"] == f["arena_R"]
    r.close()


def case_refuse():
    """Budget 1 MiB, below everything: bj_prove_async itself is out of memory, names both byte counts, hands out no ticket."""
    r = Run(10, lambda f: 1 << 20)
    f = r.f
    try:
        t = r.s.prove_async()
    except r.E.BoojumHipError as e:
        msg = str(e)
        print("refused: %s" % msg)
        numbers = [int(x) for x in re.findall(r"\d{4,}", msg)]
        assert "out of device memory" in msg and "BJ_HBM_BUDGET_BYTES" in msg
        assert numbers[0] == f["Ln"] and numbers[1] == (1 << 20) - f["tables"], numbers   # once the parent has released all but its tables
    else:
        raise AssertionError("a ticket came back: %r" % t)
    same(r.s.prove()[0], r.ref)
    r.close()


def case_no_budget():
    """No switch: two resident lanes, each the footprint R."""
    r = Run(10, None)
    f = r.f
    reserved, grew = r.async_proofs(6)
    assert reserved == [f["arena_R"]] * 6
    parent = r.free0 - r.free1
    print("two lanes took %d bytes, 2 R = %d" % (grew - parent, 2 * f["R"]))
    assert 2 * f["R"] <= grew - parent <= 2 * f["R"] + 2 * SLACK
    r.close()


def case_tickets():
    """A ticket is good for one wait; one that was never issued or whose context is gone is refused before it is read."""
    r = Run(10, None)
    E, lib, s = r.E, r.ctx._lib, r.s
    INVALID = -1
    t = s.prove_async()
    handle = C.c_void_p(t.handle.value)
    same(s.wait(t)[0], r.ref)
    h = C.c_void_p()
    assert lib.bj_proof_wait(handle, C.byref(h)) == INVALID and not h.value
    assert lib.bj_proof_poll(handle) == INVALID
    for call in (s.wait, s.done):
        try:
            call(t)
        except E.BoojumHipError as e:
            print("second use: %s" % e)
        else:
            raise AssertionError("a ticket was used twice")
    never = (C.c_uint64 * 64)()            # memory that is no ticket: looked up, not read
    assert lib.bj_proof_wait(C.cast(never, C.c_void_p), C.byref(h)) == INVALID and lib.bj_proof_poll(C.cast(never, C.c_void_p)) == INVALID
    ctx2 = E.Context(0)
    s2 = E.ProverSetup(ctx2, r.c, FRI, CAP, SEC)
    t2 = s2.prove_async()
    handle2 = C.c_void_p(t2.handle.value)
    ctx2.close()                           # bj_ctx_destroy with a proof nobody waited for: it finishes, then goes with its ticket
    assert lib.bj_proof_poll(handle2) == INVALID
    assert lib.bj_proof_wait(handle2, C.byref(h)) == INVALID and not h.value
    try:
        s2.wait(t2)
    except E.BoojumHipError as e:
        print("wait after close: %s" % e)
    else:
        raise AssertionError("wait() after ctx.close() returned")
    s2.close()
    same(s.wait(s.prove_async())[0], r.ref)   # the first context is none the worse
    r.close()


CASES = {"lane_lean": case_lane_lean, "one_lane": case_one_lane, "release_parent": case_release_parent, "refuse": case_refuse,
         "no_budget": case_no_budget, "tickets": case_tickets}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("case %s holds" % sys.argv[1])
