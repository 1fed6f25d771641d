#!/usr/bin/env python3
"""Proofs from a WitnessVec's values at the bench sizes: the gather kernel, bj_prove_values and bj_prove_values_async, on one box.

    python tools/prove_values_rate.py [--log-n 20 22] [--parent-tree DIR] [--out profiles/prove_values_rate.json]
    python tools/prove_values_rate.py --log-n 22 --from-dumps-only --tree DIR      # what the driver runs under --parent-tree

For each size the SHA-256 bench circuit is built once and a setup is made from its placement; every figure is the median of its
runs, the runs interleaved so that drift hits all sides alike:
  (a) witness_gather_kernel alone over all variable columns (bj_witness_gather on resident arrays, 5 runs): its time, and its
      fraction of the HBM peak by algorithmic bytes — 4 in, one 8-byte read, 8 out per cell — against PEAK_GBS;
  (b) bj_prove_values against bj_prove_from_dumps with a NULL hint (5 runs each, alternating).  In this tree the latter IS the
      former behind a parser; the parent commit's figure comes from the parent's own tree: check the parent out somewhere, build
      it there and pass --parent-tree, the driver then runs this script's --from-dumps-only mode on that package and library in
      child processes between its own rounds;
  (c) twenty proofs through bj_prove_values_async against twenty through bj_prove_async on pinned materialised columns with the
      `t[k] = async; wait(t[k-1])` pattern (the materialisation is not counted), 5 runs each, alternating; the spread of each side's
      five runs is reported beside the medians.
Every proof is compared with the first one: the figures are of identical proofs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_GBS = 8000.0   # MI355X HBM3E peak, GB/s
RUNS, ASYNC_PROOFS = 5, 20


def med(xs):
    return {"median_ms": statistics.median(xs), "runs_ms": xs}


def circuit(log_n):
    from era_boojum_amd import sha256_circuit as S
    t0 = time.time()
    c, info = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(log_n)), return_info=True)
    total = sum(t.shape[0] for t in S.sha_tables())
    values = np.ascontiguousarray(info["all_values"], dtype=np.uint64)
    counters = np.ascontiguousarray(c.multiplicities[0, :total].astype(np.uint32))
    print("circuit: %d x 2^%d cells, %d values, synthesis %.1f s" % (c.num_vars, c.log_n, len(values), time.time() - t0), flush=True)
    return c, np.ascontiguousarray(info["var_ids"], dtype=np.int32), values, counters


def from_dumps_ms(ctx, setup, wit, runs):
    import ctypes as C
    out = []
    for _ in range(runs):
        h = C.c_void_p()
        t = time.perf_counter()
        ctx._check(setup._lib.bj_prove_from_dumps(ctx._h, setup._h, wit, len(wit), None, 0, None, 0, C.byref(h)))
        out.append((time.perf_counter() - t) * 1e3)
        setup._finish(h)
    return out


def measure(log_n, parent_tree, dumps_only):
    try:
        import torch
        torch.cuda.init()
    except Exception:
        torch = None
    import era_boojum_amd as E
    from era_boojum_amd import memcopy_format as M
    c, var_ids, values, counters = circuit(log_n)
    V, n = var_ids.shape
    ctx = E.Context(0)
    setup = E.ProverSetup.from_placement(ctx, c, var_ids, 8, 16, 100)
    wit = M.write_witness_vec([], values, counters)
    if dumps_only:                       # a child of the driver, on the package and library of --tree
        from_dumps_ms(ctx, setup, wit, 1)
        print("FROM_DUMPS_MS " + json.dumps(from_dumps_ms(ctx, setup, wit, RUNS)), flush=True)
        return None
    res = {"log_n": log_n, "num_vars": V, "cells": V * n, "n_values": len(values), "values_bytes": values.nbytes,
           "columns_bytes": 8 * (V + 1) * n}
    # (a) the kernel alone
    place = np.where(var_ids >= 0, var_ids.astype(np.uint32), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    d_place = ctx.upload(np.ascontiguousarray(place).reshape(-1).view(np.uint64))
    d_vals, d_cells = ctx.upload(values), ctx.malloc(8 * V * n)
    assert not ctx.witness_gather(d_place, V, log_n, d_vals, len(values), d_cells)
    assert np.array_equal(ctx.d2h(d_cells, (V, n)), c.variables), "the gather differs from the circuit's columns"
    ks = []
    for _ in range(RUNS):
        ctx.timer_start()
        # the timer's events bracket the flag's memset, the one launch and the 4-byte read of the flag
        ctx.witness_gather(d_place, V, log_n, d_vals, len(values), d_cells)
        ks.append(ctx.timer_stop_ms())
    for d in (d_place, d_vals, d_cells):
        ctx.free(d)
    res["gather"] = med(ks)
    res["gather"]["algorithmic_bytes"] = 20 * V * n
    res["gather"]["fraction_of_hbm_peak"] = 20 * V * n / (res["gather"]["median_ms"] * 1e-3) / (PEAK_GBS * 1e9)
    # (b) serial: bj_prove_values against bj_prove_from_dumps with a NULL hint
    first = setup.prove_values(values, counters)[0]          # warm-up: workspace, staging
    a, b, p = [], [], []
    for _ in range(RUNS):
        t = time.perf_counter()
        proof = setup.prove_values(values, counters)[0]
        a.append((time.perf_counter() - t) * 1e3)
        assert np.array_equal(proof, first)
        b += from_dumps_ms(ctx, setup, wit, 1)
        if parent_tree:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--log-n", str(log_n), "--from-dumps-only", "--tree", parent_tree],
                               capture_output=True, text=True, check=True)
            p += json.loads([l for l in r.stdout.splitlines() if l.startswith("FROM_DUMPS_MS ")][-1].split(" ", 1)[1])
    res["prove_values"], res["prove_from_dumps_null_hint"] = med(a), med(b)
    if p:
        res["parent_prove_from_dumps_null_hint"] = med(p)
    # (c) twenty proofs pipelined, either way
    cols = np.ascontiguousarray(c.variables)
    mult = np.ascontiguousarray(c.multiplicities)
    if torch is not None:                 # pinned, as the README asks of a host of bj_prove_async
        tc, tm = torch.from_numpy(cols).pin_memory(), torch.from_numpy(mult).pin_memory()
        cols, mult = tc.numpy(), tm.numpy()

    def pipelined(submit):
        t, prev = time.perf_counter(), None
        for _ in range(ASYNC_PROOFS):
            cur = submit()
            if prev is not None:
                assert np.array_equal(setup.wait(prev)[0], first)
            prev = cur
        assert np.array_equal(setup.wait(prev)[0], first)
        return (time.perf_counter() - t) * 1e3
    sides = {"prove_values_async": lambda: setup.prove_values_async(values, counters),
             "prove_async": lambda: setup.prove_async(variables=cols, multiplicities=mult)}
    for fn in sides.values():
        pipelined(fn)                     # warm-up: both lanes reserved for either footprint
    runs = {k: [] for k in sides}
    for _ in range(RUNS):
        for k, fn in sides.items():
            runs[k].append(pipelined(fn))
    for k in sides:
        res[k + "_20_proofs"] = med(runs[k])
        res[k + "_20_proofs"]["spread_ms"] = max(runs[k]) - min(runs[k])
    res["async_difference_ms"] = res["prove_values_async_20_proofs"]["median_ms"] - res["prove_async_20_proofs"]["median_ms"]
    setup.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, for (b)")
    ap.add_argument("--from-dumps-only", action="store_true")
    ap.add_argument("--tree", default=None, help="import era_boojum_amd from this checkout instead of the script's own")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    out = []
    for log_n in args.log_n:
        r = measure(log_n, args.parent_tree, args.from_dumps_only)
        if r is not None:
            print(json.dumps(r), flush=True)
            out.append(r)
    if args.out and out:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        with open(args.out, "w") as f:
            f.write(json.dumps({"measured_on_commit": commit, "peak_gbs": PEAK_GBS, "sizes": out}, indent=1) + "\n")


if __name__ == "__main__":
    main()
