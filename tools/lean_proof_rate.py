#!/usr/bin/env python3
"""What a lean proof (BJ_PROOF_LEAN) costs in time and saves in workspace, resident and lean proofs of the SHA-256
bench circuit interleaved in one process on one resident setup.

    python tools/lean_proof_rate.py [--log-n 20 22] [--runs 5] [--out profiles/lean_proof_rate.json] [--label "<commit>, <box>"]

Per trace length: the reserved and high-water workspace bytes of either mode (each from a proof on a released arena); per-proof
wall times of bj_prove_dev on the resident witness, resident and lean alternating, their medians, and the medians of every stage
of bj_proof_stage_ms; and the three predictors, measured here and never taken from the prover:
  quotient stage   q one-coset bj_lde_cosets_batch runs of nW + nS2 columns, the transforms the lean quotient round adds;
  query stage      the lean-setup figure (13.3 ms for 105 columns and 34 queries at 2^22 rows) scaled by (nW + nS2) / 105;
  host witness     bj_prove through pinned memory, resident against lean: the overlap of hashing with PCIe that the lean mode gives up.
The lean proof is checked to be the resident proof's bytes."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LEAN_SETUP_QUERY_MS, LEAN_SETUP_COLUMNS, LEAN_SETUP_LOG_N = 13.3, 105, 22   # DESIGN.md §5, the lean-setup entry


def measure(E, ctx, log_n, runs):
    import torch
    from era_boojum_amd import binding, proof_format, sha256_circuit as S
    t0 = time.time()
    c = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(log_n)))
    n = 1 << c.log_n
    print("circuit: %d x 2^%d cells, synthesis %.1f s" % (c.num_vars, c.log_n, time.time() - t0), flush=True)
    setup = E.ProverSetup(ctx, c, 8, 16, 100)
    q = c.quotient_degree
    d_v, d_m = ctx.upload(c.variables), ctx.upload(c.multiplicities)
    modes = (("resident", False), ("lean", True))

    def proof(on, host=None):
        with ctx.lean_proofs(on):
            ctx.sync()
            t = time.perf_counter()
            buf, stages = setup.prove(*host) if host else setup.prove_dev(d_v, d_m)
            return (time.perf_counter() - t) * 1e3, buf, stages

    workspace = {}
    ctx.release_workspace()              # the arena only grows: the smaller mode first, each from a released arena
    _, got, _ = proof(True)
    workspace["lean"] = dict(setup.last_workspace)
    ctx.release_workspace()
    _, ref, _ = proof(False)
    workspace["resident"] = dict(setup.last_workspace)
    assert np.array_equal(ref, got), "the lean proof is not the resident proof"
    nW, nS2 = int(ref[10]), int(ref[11])
    times = {k: [] for k, _ in modes}
    stages = {k: [] for k, _ in modes}
    for _ in range(runs):
        for name, on in modes:
            ms, _, st = proof(on)
            times[name].append(ms)
            stages[name].append(st)
    med = {k: statistics.median(v) for k, v in times.items()}
    stage_names = list(binding.STAGE_NAMES) + ["witness_tree_leaf_kernel"]
    stage_med = {k: {s: statistics.median(x[s] for x in v) for s in stage_names} for k, v in stages.items()}
    overhead = {s: stage_med["lean"][s] - stage_med["resident"][s] for s in stage_names}
    # predictor 1: nW + nS2 columns through bj_lde_cosets_batch, one coset per call, q calls
    tiled = bool(ctx.monomials_tiled(c.log_n))
    cols = nW + nS2
    d_mono, d_out = ctx.malloc(8 * cols * n), ctx.malloc(8 * cols * n)   # whatever words they hold: the transform's time does not depend on them
    lde = ctx.lde_cosets_batch_tiled if tiled else ctx.lde_cosets_batch
    log_lde = (max(8, q) - 1).bit_length()
    lde_runs = []
    for _ in range(runs + 1):
        ctx.sync()
        t = time.perf_counter()
        for coset in range(q):
            lde(d_mono, d_out, c.log_n, cols, log_lde, coset, 1)
        ctx.sync()
        lde_runs.append((time.perf_counter() - t) * 1e3)
    lde_runs = lde_runs[1:]
    ctx.free(d_mono)
    ctx.free(d_out)
    # predictor 3: bj_prove, the witness in pinned host memory
    hv = torch.from_numpy(c.variables.view(np.int64)).pin_memory().numpy().view(np.uint64)
    hm = torch.from_numpy(c.multiplicities.view(np.int64)).pin_memory().numpy().view(np.uint64)
    host_times = {k: [] for k, _ in modes}
    for name, on in modes:               # staging allocation, first touch
        _, buf, _ = proof(on, (hv, hm))
        assert np.array_equal(buf, ref)
    for _ in range(runs):
        for name, on in modes:
            host_times[name].append(proof(on, (hv, hm))[0])
    host_med = {k: statistics.median(v) for k, v in host_times.items()}
    queries = len(proof_format.parse(ref, security_level=100)["_query_indices"])
    res = {"log_n": c.log_n, "num_vars": c.num_vars, "witness_columns": nW, "stage2_columns": nS2, "quotient_degree": q, "monomials_tiled": tiled,
           "queries": queries, "workspace_bytes": workspace,
           "reserved_bytes_saved": workspace["resident"]["reserved_bytes"] - workspace["lean"]["reserved_bytes"],
           "prove_dev_ms": med, "prove_dev_runs_ms": times, "lean_costs_ms": med["lean"] - med["resident"],
           "stage_ms": stage_med, "stage_overhead_ms": overhead,
           "quotient_stage": {"overhead_ms": overhead["quotient_work_and_lde"], "predicted_by_lde_cosets_batch_ms": statistics.median(lde_runs),
                              "lde_cosets_batch_runs_ms": lde_runs},
           "query_stage": {"overhead_ms": overhead["queries"],
                           "predicted_from_lean_setup_ms": LEAN_SETUP_QUERY_MS * cols / LEAN_SETUP_COLUMNS if c.log_n == LEAN_SETUP_LOG_N else None},
           "host_witness": {"bj_prove_ms": host_med, "bj_prove_runs_ms": host_times, "lean_costs_ms": host_med["lean"] - host_med["resident"],
                            "overlap_lost_ms": (host_med["lean"] - host_med["resident"]) - (med["lean"] - med["resident"])}}
    for p in (d_v, d_m):
        ctx.free(p)
    setup.close()
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
    res = {"what": "resident against lean proofs (BJ_PROOF_LEAN): bj_prove_dev and bj_prove of the SHA-256 bench circuit on one resident setup, "
                   "interleaved in one process, measured on this run", "measured_on": args.label, "sizes": []}
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
