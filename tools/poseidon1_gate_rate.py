#!/usr/bin/env python3
"""Quotient launch of the Poseidon (v1) flattened gate (PoseidonFlattenedGate<8,12,4>) on one MI355X: every arm is ONE
bj_quotient_gates call in quotient mode (selector path of 2, alpha-weighted sum of the 118 terms) over the same --log-points
points (default 2^22 rows x LDE 8 = 2^25):
  hand_written     kind BJ_GATE_POSEIDON_FLATTENED (csrc/gate_poseidon.hip)
  capture_routed   the reference's op-list capture as kind BJ_GATE_PROGRAM: its fingerprint selects the same kernel
  hiprtc           gate_program.poseidon_flattened_compact_program() as an op list: the same 118 terms, a fingerprint no table
                   knows, so its kernel is compiled at run time (checked: bj_gate_jit_status counts one more kernel)
  interpreter      the reference's capture with BJ_GATE_NO_AOT=1 (no build-time or hand-written kernel; a known fingerprint is
                   never sent to the run-time compiler), in a child process because the switch is read once per process
Each arm: one warm-up call, then --reps timed calls.  Prints one JSON object (and writes it to --out).
    python tools/poseidon1_gate_rate.py [--log-points 25] [--reps 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(xs, points):
    med = statistics.median(xs)
    return {"median_ms": round(med, 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "n": len(xs),
            "ns_per_point": round(med * 1e6 / points, 4)}


def _jit_count():
    import era_boojum_amd as E
    buf = C.create_string_buffer(512)
    return E.load_library().bj_gate_jit_status(buf, 512), buf.value.decode(errors="replace")


class _Arm:
    def __init__(self, ctx, log_points):
        import torch
        dev = torch.device("cuda", 0)
        self.ctx, self.Q = ctx, 1 << log_points
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        self.var = torch.randint(-2**63, 2**63 - 1, (130, self.Q), dtype=torch.int64, device=dev, generator=g)
        self.con = torch.randint(-2**63, 2**63 - 1, (2, self.Q), dtype=torch.int64, device=dev, generator=g)
        self.out = torch.empty((2, self.Q), dtype=torch.int64, device=dev)
        self.alphas = [[3 + k, 5 + k] for k in range(118)]

    def time(self, gate, reps):
        Q = self.Q

        def one():
            self.ctx.timer_start()
            self.ctx.quotient_gates(self.var.data_ptr(), Q, 130, self.con.data_ptr(), Q, 2, [gate], self.alphas, Q,
                                    self.out.data_ptr(), self.out.data_ptr() + 8 * Q)
            return self.ctx.timer_stop_ms()
        one()
        return _stats([one() for _ in range(reps)], Q)

    def result(self):
        return self.out.cpu().numpy()


def _gate(kind, program=None):
    from era_boojum_amd import synthetic as S
    return S.GateDesc(kind, "PoseidonFlattenedGate", 7, 0, 130, 1, 130, 0, 118, True, path=[True, False], program=program)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-points", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--interpreter-arm", action="store_true")      # the child process (BJ_GATE_NO_AOT=1)
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import era_boojum_amd as E
    from era_boojum_amd import gate_program as G, synthetic as S
    ctx = E.Context(0)
    arm = _Arm(ctx, a.log_points)
    if a.interpreter_arm:
        assert os.environ.get("BJ_GATE_NO_AOT") == "1"
        r = arm.time(_gate(S.GATE_PROGRAM, G.poseidon_flattened_program()), a.reps)
        r["jit_kernels_in_process"] = _jit_count()[0]
        np.save(os.environ["P1_RATE_OUT"], arm.result())
        print(json.dumps(r))
        return
    capture, compact = G.poseidon_flattened_program(), G.poseidon_flattened_compact_program()
    lib = E.load_library()
    assert lib.bj_gate_program_generated(C.byref(capture.struct)) == 1 and lib.bj_gate_program_generated(C.byref(compact.struct)) == 0
    res = {"points": arm.Q, "what": "one bj_quotient_gates launch, quotient mode, selector path of 2"}
    res["hand_written"] = arm.time(_gate(S.GATE_POSEIDON_FLATTENED), a.reps)
    want = arm.result()
    res["capture_routed"] = arm.time(_gate(S.GATE_PROGRAM, capture), a.reps)
    assert np.array_equal(arm.result(), want)
    before = _jit_count()[0]
    res["hiprtc"] = arm.time(_gate(S.GATE_PROGRAM, compact), a.reps)
    n_jit, status = _jit_count()
    if n_jit <= before:
        raise SystemExit("the run-time compiler did not produce a kernel for the compact program: " + status)
    res["hiprtc"]["jit_status"] = status
    assert np.array_equal(arm.result(), want)
    del arm
    torch.cuda.empty_cache()
    fd, tmp = tempfile.mkstemp(suffix=".npy")
    os.close(fd)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--interpreter-arm", "--log-points", str(a.log_points), "--reps",
                        str(a.reps)], env=dict(os.environ, BJ_GATE_NO_AOT="1", P1_RATE_OUT=tmp), capture_output=True, text=True,
                       timeout=900)
    if r.returncode:
        raise SystemExit("interpreter arm failed:\n" + r.stderr[-2000:])
    res["interpreter"] = json.loads(r.stdout.strip().splitlines()[-1])
    if res["interpreter"]["jit_kernels_in_process"]:
        raise SystemExit("the interpreter arm obtained a run-time compiled kernel")
    assert np.array_equal(np.load(tmp), want)
    os.remove(tmp)
    hw = res["hand_written"]["median_ms"]
    res["time_ratio_to_hand_written"] = {k: round(res[k]["median_ms"] / hw, 2) for k in ("capture_routed", "hiprtc", "interpreter")}
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
