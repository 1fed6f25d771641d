#!/usr/bin/env python3
"""bj_check_copy_constraints at the bench size, next to bj_check_satisfied on the same setup, on one box in one process.

    python tools/copy_check_rate.py [--log-n 22] [--out profiles/copy_check_2p22.json]

Builds the SHA-256 bench circuit once, keeps the witness resident, and takes the median of 3 runs (wall clock around the
synchronous call) of
  (a) bj_check_copy_constraints on the honest witness (one pass: decode every sigma word, mark its target, compare two values);
  (b) the same with one cell of a copy cycle changed (the named cell's sigma word is decoded once more on the host);
  (c) bj_sigma_cells over the setup-sized sigma columns: the decoding alone, with its 4-byte store per cell (device events);
  (d) bj_check_satisfied on the same setup, the yardstick (existing code)."""
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
    V, n, log_n = c.num_vars, 1 << c.log_n, c.log_n
    print("circuit: %d x 2^%d cells, synthesis %.1f s" % (V, log_n, time.time() - t0), flush=True)
    setup = E.ProverSetup(ctx, c, 8, 16, 100)
    # a cell of column 0 in a copy cycle: the first row where sigma[0] is not the cell's own identity
    from era_boojum_amd import field_np as F
    ident0 = F.mul(F.powers(F.omega(log_n), n), np.uint64(c.non_residues[0]))
    row = int(np.flatnonzero(c.sigmas[0] != ident0)[0])
    broken = np.array(c.variables, dtype=np.uint64)
    broken[0, row] = (int(broken[0, row]) + 1) % E.P
    d_good, d_bad, d_m = ctx.upload(c.variables), ctx.upload(broken), ctx.upload(c.multiplicities)
    d_sig, d_cells = ctx.upload(c.sigmas), ctx.malloc(4 * V * n)

    def timed(fn):
        def run():
            ctx.sync()
            t = time.perf_counter()
            fn()
            return (time.perf_counter() - t) * 1e3
        return run

    def decode_only():
        ctx.timer_start()
        out = ctx.sigma_cells(d_sig, V, log_n, c.non_residues, d_cells)
        ms = ctx.timer_stop_ms()
        assert out == (None, 0), out
        return ms
    reports = {}
    setup.check_copy_constraints(d_good)             # first call: the scratch allocation
    ok_ms, ok_all = median3(timed(lambda: reports.__setitem__("ok", setup.check_copy_constraints(d_good))))
    bad_ms, bad_all = median3(timed(lambda: reports.__setitem__("bad", setup.check_copy_constraints(d_bad))))
    assert reports["ok"].kind == E.binding.COPY_OK and reports["ok"].failures == (0, 0, 0, 0), str(reports["ok"])
    r = reports["bad"]
    assert r.kind == E.binding.COPY_VALUE_MISMATCH and r.failures[3] == 2 and (0, row) in ((r.column, r.row), (r.partner_column, r.partner_row)), str(r)
    decode_only()
    dec_ms, dec_all = median3(decode_only)
    setup.check_satisfied_dev(d_good, d_m)
    sat_ms, sat_all = median3(timed(lambda: reports.__setitem__("sat", setup.check_satisfied_dev(d_good, d_m))))
    assert reports["sat"].kind == E.binding.SAT, str(reports["sat"])
    rounds = [(i, min(4, log_n - i)) for i in range(0, log_n, 4)]
    products = log_n + 1 + sum(log_n - i - w + 1 for i, w in rounds)
    res = {"what": "bj_check_copy_constraints next to bj_check_satisfied, real SHA-256 circuit, witness resident, median of 3, measured on this run",
           "log_n": log_n, "num_vars": V, "cells": V * n, "row_method": "plain Pohlig-Hellman, 4 bits per round", "products_per_cell": products,
           "check_copy_constraints_ms": ok_ms, "check_copy_constraints_runs_ms": ok_all,
           "check_one_changed_cell_ms": bad_ms, "check_one_changed_cell_runs_ms": bad_all, "changed_report": str(r),
           "sigma_cells_ms": dec_ms, "sigma_cells_runs_ms": dec_all,
           "check_satisfied_ms": sat_ms, "check_satisfied_runs_ms": sat_all, "copy_over_satisfied": ok_ms / sat_ms}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for p in (d_good, d_bad, d_m, d_sig, d_cells):
        ctx.free(p)
    setup.close()
    ctx.close()


if __name__ == "__main__":
    main()
