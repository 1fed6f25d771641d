#!/usr/bin/env python3
"""bj_lookup_multiplicities at the bench size, and what counting the column costs a proof, on one box in one process.

    python tools/lookup_multiplicities_rate.py [--log-n 22] [--out profiles/lookup_multiplicities_rate.json] [--label "<commit>, <box>"]

Builds the SHA-256 bench circuit once and keeps the witness resident.  Three lookup distributions of the same shape:
  real      the circuit's own lookup columns (skewed: the unused sub-arguments all look one tuple up);
  uniform   every (sub-argument, row) looks a uniformly drawn real table row up;
  one_row   every (sub-argument, row) looks the same table row up.
For each, the median of 3 synchronous calls (wall clock) with all sub-arguments and with the first sub-argument alone: the
difference, scaled by reps / (reps - 1), is the count; the rest is the fixed part (two memsets, index build, materialise, the
read-back of the miss count).  The achieved fraction is the algorithmic bytes n * reps * (width + 1) * 8 of the count against
8 TB/s.  For the real circuit the proof's own probes (bj_proof_kernel_stats: lookup_index_build, lookup_count) are recorded too,
and bj_prove_dev without a column is timed against bj_prove_dev with a resident supplied column (median of 5 each, interleaved)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="", help="commit and box the figures were measured on")
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
    n, w, reps, cps = 1 << c.log_n, c.lookup_width, c.lookup_reps, c.lookup_cols_per_sub
    print("circuit: %d x 2^%d cells, synthesis %.1f s" % (c.num_vars, c.log_n, time.time() - t0), flush=True)
    setup = E.ProverSetup(ctx, c, 8, 16, 100)
    d_v, d_m, d_out = ctx.upload(c.variables), ctx.upload(c.multiplicities), ctx.malloc(8 * n)
    d_tables = ctx.upload(c.tables)
    d_tid = None if c.table_id_as_variable else ctx.upload(c.constants[c.table_id_col])

    def timed(fn, runs=3):
        out = []
        for _ in range(runs):
            ctx.sync()
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return statistics.median(out), out

    def rate(d_lvars):
        call = lambda r: ctx.lookup_multiplicities(d_lvars, n, d_tid, d_tables, n, r, w, c.log_n, d_out)   # noqa: E731
        call(reps)                                   # first call: the scratch allocation
        one_ms, _ = timed(lambda: call(1))
        all_ms, all_runs = timed(lambda: call(reps))     # last: d_out holds the whole column afterwards
        count_ms = (all_ms - one_ms) * reps / (reps - 1) if reps > 1 else float("nan")
        algorithmic = n * reps * (w + 1) * 8
        return {"call_ms": all_ms, "call_runs_ms": all_runs, "first_sub_argument_alone_ms": one_ms, "count_ms": count_ms,
                "fixed_ms": all_ms - count_ms, "algorithmic_bytes": algorithmic,
                "count_fraction_of_8TBps": algorithmic / (count_ms * 1e-3) / HBM_BYTES_PER_S if count_ms > 0 else None}

    res = {"what": "bj_lookup_multiplicities and bj_prove_dev without a multiplicity column, real SHA-256 circuit, witness resident, "
                   "measured on this run", "measured_on": args.label, "log_n": c.log_n, "num_vars": c.num_vars, "lookup_reps": reps,
           "lookup_width": w, "table_rows": int(c.total_tables_len), "distributions": {}}
    lo = c.num_gp_vars * n * 8
    res["distributions"]["real"] = rate(d_v + lo)
    assert np.array_equal(ctx.d2h(d_out, (1, n)), c.multiplicities), "the counted column is not the circuit's"
    rng = np.random.default_rng(1)
    for name, pick in (("uniform", rng.integers(0, c.total_tables_len, size=(reps, n))), ("one_row", np.zeros((reps, n), dtype=np.int64))):
        lv = np.empty((reps * cps, n), dtype=np.uint64)
        for sub in range(reps):
            for j in range(cps):
                lv[sub * cps + j] = c.tables[j][pick[sub]]
        if d_tid is not None:                        # the id comes from the constant column: draw within the row's own table
            ids = np.asarray(c.constants[c.table_id_col], dtype=np.uint64)
            by_id = {int(t): np.flatnonzero(c.tables[w] == t) for t in np.unique(ids)}
            for sub in range(reps):
                rows = np.empty(n, dtype=np.int64)
                for t, cand in by_id.items():
                    m = ids == t
                    rows[m] = cand[0] if name == "one_row" else cand[rng.integers(0, len(cand), size=int(m.sum()))]
                for j in range(w):
                    lv[sub * cps + j] = c.tables[j][rows]
        d_lv = ctx.upload(lv)
        res["distributions"][name] = rate(d_lv)
        ctx.free(d_lv)

    stages = {}
    setup.prove_dev(d_v, d_m)                        # first proofs: the workspace reservation, with and without the column
    ref, _ = setup.prove_dev(d_v, None, count_multiplicities=True)
    probes = {k: {"ms": v[0], "algorithmic_bytes": v[1], "fraction_of_8TBps": v[1] / (v[0] * 1e-3) / HBM_BYTES_PER_S}
              for k, v in setup.last_kernels.items() if k.startswith("lookup_")}
    supplied, counted = [], []
    for _ in range(5):
        ms, _ = timed(lambda: stages.update(setup.prove_dev(d_v, d_m)[1]), runs=1)
        supplied.append(ms)
        ms, _ = timed(lambda: setup.prove_dev(d_v, None, count_multiplicities=True), runs=1)
        counted.append(ms)
    assert np.array_equal(ref, setup.prove_dev(d_v, d_m)[0]), "the proof without a column differs"
    pcie_ms = n * 8 / 50e9 * 1e3                     # the column it replaces at ~50 GB/s of pinned PCIe 5 x16
    res.update({"proof_probes": probes, "prove_dev_supplied_ms": statistics.median(supplied), "prove_dev_supplied_runs_ms": supplied,
                "prove_dev_counted_ms": statistics.median(counted), "prove_dev_counted_runs_ms": counted,
                "counting_costs_ms": statistics.median(counted) - statistics.median(supplied),
                "column_bytes": n * 8, "column_pcie_copy_ms_at_50GBps": pcie_ms})
    res["counting_costs_more_than_the_copy"] = res["counting_costs_ms"] > pcie_ms
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for p in (d_v, d_m, d_out, d_tables, d_tid):
        if p is not None:
            ctx.free(p)
    setup.close()
    ctx.close()


if __name__ == "__main__":
    main()
