#!/usr/bin/env python3
"""bj_list_unsatisfied next to bj_check_satisfied (unchanged code: the yardstick) on one box in one process.

    python tools/list_unsatisfied_rate.py [--log-n 10 20] [--out profiles/list_unsatisfied.json]

Per size a synthetic SHA-shaped circuit (sha_shaped_circuit, table_bits=2; 2^10 is the suite's sha10), witness and multiplicities
resident, wall clock around the synchronous C call (the checker through its binding method, which builds one small report):
  (a) five runs of the checker and five of the listing on the satisfied witness (the checker's spread is what the difference of
      the medians is read against);
  (b) the listing on the dense family — general-purpose variable column 0 changed on every row — at capacity 64 and 2^16, median
      of 3, with the totals it returns, and at 2^16 once more through the binding, which builds one Python record per entry;
  (c) the scratch the listing takes: free HBM before and after the first call on a context whose workspace was released."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import era_boojum_amd as E
    from era_boojum_amd import synthetic as S
    ctx = E.Context(0)

    def timed(fn, runs):
        out = []
        for _ in range(runs):
            ctx.sync()
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return out

    def raw_call(setup, d_v, d_m, capacity):
        """the C call alone, into a buffer made once: the binding's records (one Python object per entry) stay out of the time"""
        import ctypes as C
        buf, n, totals = (E.binding._UnsatEntry * capacity)(), C.c_size_t(0), (C.c_uint64 * 5)()

        def run():
            assert setup._lib.bj_list_unsatisfied(ctx._h, setup._h, d_v, d_m, buf, capacity, C.byref(n), totals) == 0
        return run
    sizes = []
    for log_n in args.log_n:
        c = S.sha_shaped_circuit(log_n, seed=11, table_bits=2)
        n = 1 << log_n
        setup = E.ProverSetup(ctx, c, 8, 16, 30)
        dense = np.array(c.variables, dtype=np.uint64)
        dense[0] = (dense[0] + np.uint64(1)) % np.uint64(E.P)
        d_good, d_bad, d_m = ctx.upload(c.variables), ctx.upload(dense), ctx.upload(c.multiplicities)
        ctx.release_workspace()
        ctx.sync()
        free_before = torch.cuda.mem_get_info()[0]
        first = setup.list_unsatisfied_dev(d_bad, d_m, 1 << 16)      # first call: the scratch allocation
        ctx.sync()
        scratch = free_before - torch.cuda.mem_get_info()[0]
        setup.check_satisfied_dev(d_good, d_m)
        check_runs = timed(lambda: setup.check_satisfied_dev(d_good, d_m), 5)
        list_runs = timed(raw_call(setup, d_good, d_m, 64), 5)
        assert setup.list_unsatisfied_dev(d_good, d_m, 64) == ([], (0, 0, 0, 0, 0))
        dense_64 = timed(raw_call(setup, d_bad, d_m, 64), 3)
        dense_64k = timed(raw_call(setup, d_bad, d_m, 1 << 16), 3)
        dense_64k_py = timed(lambda: setup.list_unsatisfied_dev(d_bad, d_m, 1 << 16), 3)
        check_dense = timed(lambda: setup.check_satisfied_dev(d_bad, d_m), 3)
        entries, totals = setup.list_unsatisfied_dev(d_bad, d_m, 64)
        rep = setup.check_satisfied_dev(d_bad, d_m)
        assert totals == first[1] and len(entries) == min(64, totals[0]) and entries[0].row == rep.row and totals[1] >= rep.failures[1]
        sizes.append({"log_n": log_n, "num_vars": c.num_vars, "lookup_reps": c.lookup_reps,
                      "satisfied_check_runs_ms": check_runs, "satisfied_check_ms": statistics.median(check_runs),
                      "satisfied_check_spread_ms": max(check_runs) - min(check_runs),
                      "satisfied_list_runs_ms": list_runs, "satisfied_list_ms": statistics.median(list_runs),
                      "dense_totals": list(totals), "dense_flagged_rows": rep.failures[1],
                      "dense_list_capacity_64_ms": statistics.median(dense_64), "dense_list_capacity_64_runs_ms": dense_64,
                      "dense_list_capacity_65536_ms": statistics.median(dense_64k), "dense_list_capacity_65536_runs_ms": dense_64k,
                      "dense_list_capacity_65536_with_python_records_ms": statistics.median(dense_64k_py),
                      "dense_check_ms": statistics.median(check_dense),
                      "list_scratch_bytes": int(scratch)})
        print(json.dumps(sizes[-1]), flush=True)
        for p in (d_good, d_bad, d_m):
            ctx.free(p)
        setup.close()
    res = {"what": "bj_list_unsatisfied next to bj_check_satisfied, sha_shaped_circuit(seed=11, table_bits=2), witness resident, wall clock "
                   "around the synchronous call, measured on this run", "sizes": sizes}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
