#!/usr/bin/env python3
"""What a lean setup (BJ_SETUP_LEAN) costs a proof and saves in HBM, resident and lean proofs of the SHA-256 bench
circuit interleaved in one process.

    python tools/lean_setup_rate.py [--log-n 20 22] [--runs 5] [--out profiles/lean_setup_rate.json] [--label "<commit>, <box>"]

Per trace length: both bj_setup_device_bytes; per-proof wall times of bj_prove_dev on the resident witness, resident and lean
alternating (first proofs of either kind discarded: workspace reservation), their medians; bj_proof_stage_ms of the quotient and
query stages of both; the time of bj_lde_cosets_batch of the setup's column count over the quotient's q cosets, taken one coset per
call as the lean quotient round takes them — the prediction of the quotient stage's overhead; and the query stage's difference,
which is eval_monomials_at_kernel against gather_rows.  The lean proof is checked to be the resident proof's bytes."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def measure(E, ctx, log_n, runs):
    from era_boojum_amd import proof_format, sha256_circuit as S
    t0 = time.time()
    c = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(log_n)))
    n = 1 << c.log_n
    print("circuit: %d x 2^%d cells, synthesis %.1f s" % (c.num_vars, c.log_n, time.time() - t0), flush=True)
    resident = E.ProverSetup(ctx, c, 8, 16, 100)
    lean = E.ProverSetup(ctx, c, 8, 16, 100, lean=True)
    n_cols = c.num_vars + c.num_constant_cols + (c.tables.shape[0] if c.lookup_reps else 0)
    q = c.quotient_degree
    d_v, d_m = ctx.upload(c.variables), ctx.upload(c.multiplicities)

    def proof(s):
        ctx.sync()
        t = time.perf_counter()
        buf, stages = s.prove_dev(d_v, d_m)
        return (time.perf_counter() - t) * 1e3, buf, stages

    _, ref, _ = proof(resident)          # the first of each kind: workspace reservation (the lean plan is the larger one)
    _, got, _ = proof(lean)
    assert np.array_equal(ref, got), "the lean proof is not the resident proof"
    proof(resident)
    times = {"resident": [], "lean": []}
    stages = {"resident": [], "lean": []}
    for _ in range(runs):
        for name, s in (("resident", resident), ("lean", lean)):
            ms, _, st = proof(s)
            times[name].append(ms)
            stages[name].append(st)
    med = {k: statistics.median(v) for k, v in times.items()}
    stage_med = {k: {s: statistics.median(x[s] for x in v) for s in ("quotient_work_and_lde", "queries")} for k, v in stages.items()}
    # the predictor: the setup's column count through bj_lde_cosets_batch, one coset per call, q calls
    tiled = bool(ctx.monomials_tiled(c.log_n))
    d_mono, d_out = ctx.malloc(8 * n_cols * n), ctx.malloc(8 * n_cols * n)   # whatever words they hold: the transform's time does not depend on them
    lde = ctx.lde_cosets_batch_tiled if tiled else ctx.lde_cosets_batch
    log_lde = (max(8, q) - 1).bit_length()
    lde_runs = []
    for _ in range(runs + 1):
        ctx.sync()
        t = time.perf_counter()
        for coset in range(q):
            lde(d_mono, d_out, c.log_n, n_cols, log_lde, coset, 1)
        ctx.sync()
        lde_runs.append((time.perf_counter() - t) * 1e3)
    lde_runs = lde_runs[1:]
    ctx.free(d_mono)
    ctx.free(d_out)
    res = {"log_n": c.log_n, "num_vars": c.num_vars, "setup_columns": n_cols, "quotient_degree": q, "monomials_tiled": tiled,
           "queries": len(proof_format.parse(ref, security_level=100)["_query_indices"]),
           "setup_device_bytes": {"resident": resident.device_bytes(), "lean": lean.device_bytes()},
           "workspace_reserved_bytes_lean": lean.last_workspace["reserved_bytes"],
           "prove_dev_ms": med, "prove_dev_runs_ms": times, "lean_costs_ms": med["lean"] - med["resident"],
           "stage_ms": stage_med,
           "quotient_stage_overhead_ms": stage_med["lean"]["quotient_work_and_lde"] - stage_med["resident"]["quotient_work_and_lde"],
           "predicted_by_lde_cosets_batch_ms": statistics.median(lde_runs), "lde_cosets_batch_runs_ms": lde_runs,
           "query_stage_overhead_ms": stage_med["lean"]["queries"] - stage_med["resident"]["queries"]}
    res["evaluation_above_gather_plus_10pct_of_quotient"] = res["query_stage_overhead_ms"] > 0.10 * stage_med["resident"]["quotient_work_and_lde"]
    for p in (d_v, d_m):
        ctx.free(p)
    resident.close()
    lean.close()
    ctx.release_workspace()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="", help="commit and box the figures were measured on")
    args = ap.parse_args()
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    import era_boojum_amd as E
    ctx = E.Context(0)
    res = {"what": "resident against lean setups (BJ_SETUP_LEAN): bj_prove_dev of the SHA-256 bench circuit, witness resident, interleaved "
                   "in one process, measured on this run", "measured_on": args.label, "sizes": []}
    for log_n in args.log_n:
        r = measure(E, ctx, log_n, args.runs)
        print(json.dumps(r), flush=True)
        res["sizes"].append(r)
        if args.out:                     # after every size: a later one that runs out of time leaves the earlier figures
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
