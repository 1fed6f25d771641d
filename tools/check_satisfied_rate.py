#!/usr/bin/env python3
"""bj_check_satisfied at the bench size, next to one proof of the same witness, on one box in one process.

    python tools/check_satisfied_rate.py [--log-n 22] [--out profiles/check_satisfied_2p22.json]

Builds the SHA-256 bench circuit once, keeps witness and multiplicities resident, and takes the median of 3 runs (wall clock
around the synchronous call) of
  (a) the check on the satisfied witness;
  (b) the check with one cell of the last FMA row changed (phase 2 runs: one row, term by term);
  (c) bj_prove_dev, with its own quotient stage (bj_proof_stage_ms[2]) — the stage that evaluates the same gate terms at
      quotient_degree times as many points and that today is the first to notice an unsatisfied gate."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def median3(fn):
    out = [fn() for _ in range(3)]
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    import era_boojum_amd as E
    from era_boojum_amd import sha256_circuit as S
    ctx = E.Context(0)
    t0 = time.time()
    c = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(args.log_n)))
    n = 1 << c.log_n
    print("circuit: %d x 2^%d cells, synthesis %.1f s" % (c.num_vars, c.log_n, time.time() - t0), flush=True)
    setup = E.ProverSetup(ctx, c, 8, 16, 100)
    fma = [g.name for g in c.gates].index("FmaGateInBaseFieldWithoutConstant")
    rows = np.ones(n, dtype=bool)
    for i, bit in enumerate(c.gates[fma].path):
        rows &= c.constants[i] == (1 if bit else 0)
    row, g = int(np.flatnonzero(rows)[-1]), c.gates[fma]
    cell = (g.reps - 1) * g.var_stride + 3
    broken = np.array(c.variables, dtype=np.uint64)
    broken[cell, row] = (int(broken[cell, row]) + 1) % E.P
    d_good, d_bad, d_m = ctx.upload(c.variables), ctx.upload(broken), ctx.upload(c.multiplicities)

    def timed(fn):
        def run():
            ctx.sync()
            t = time.perf_counter()
            fn()
            return (time.perf_counter() - t) * 1e3
        return run
    reports = {}
    setup.check_satisfied_dev(d_good, d_m)           # first call: the scratch allocation
    sat_ms, sat_all = median3(timed(lambda: reports.__setitem__("sat", setup.check_satisfied_dev(d_good, d_m))))
    bad_ms, bad_all = median3(timed(lambda: reports.__setitem__("bad", setup.check_satisfied_dev(d_bad, d_m))))
    assert reports["sat"].kind == E.binding.SAT, str(reports["sat"])
    r = reports["bad"]
    assert (r.kind, r.gate, r.repetition, r.row) == (E.binding.UNSAT_GATE, fma, g.reps - 1, row), str(r)
    stages = {}
    setup.prove_dev(d_good, d_m)                     # first proof: the workspace reservation
    prove_ms, prove_all = median3(timed(lambda: stages.update(setup.prove_dev(d_good, d_m)[1])))
    quotient_ms = [v for k, v in stages.items() if "quotient" in k.lower()]
    res = {"what": "bj_check_satisfied next to bj_prove_dev, real SHA-256 circuit, witness resident, median of 3, measured on this run",
           "log_n": c.log_n, "num_vars": c.num_vars, "lookup_reps": c.lookup_reps,
           "check_satisfied_ms": sat_ms, "check_satisfied_runs_ms": sat_all,
           "check_one_broken_cell_ms": bad_ms, "check_one_broken_cell_runs_ms": bad_all, "broken_report": str(r),
           "prove_dev_ms": prove_ms, "prove_dev_runs_ms": prove_all, "prove_quotient_stage_ms": quotient_ms[0] if quotient_ms else None,
           "check_over_proof": sat_ms / prove_ms}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for p in (d_good, d_bad, d_m):
        ctx.free(p)
    setup.close()
    ctx.close()


if __name__ == "__main__":
    main()
