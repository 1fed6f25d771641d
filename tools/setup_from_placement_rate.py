#!/usr/bin/env python3
"""sigma from the placement at the bench size: the host's serial walk against the device operator, on one box in one process.

    python tools/setup_from_placement_rate.py [--log-n 22] [--out profiles/setup_from_placement_2p22.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/setup_from_placement_rate.py --operator-only   # per-kernel times

Builds the SHA-256 bench circuit once, checks that the device sigma equals the circuit's word for word, then takes the median of
3 runs of
  (a) host path:   synth_sigma_from_placement (the reference's create_permutation_polys loop) + upload of the sigma array;
  (b) device path: upload of the copy hint + bj_sigmas_from_placement, and its kernels alone (bj_timer_*, hint resident);
  (c) bj_prove_from_dumps on a setup made from the placement, with and without the DenseVariablesCopyHint.
Both (a) and (b) move [num_vars][n] u64 over PCIe from pageable memory, so their difference is the serial walk against the
kernels.  The identities the host walk starts from are computed outside (a)'s timed region.  The sort's share of the kernel time
comes from the rocprofv3 run (rocPRIM's kernels carry `radix` / `onesweep` in their names)."""
import argparse
import ctypes as C
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
    ap.add_argument("--operator-only", action="store_true", help="one operator call on the circuit's placement (for a kernel trace)")
    args = ap.parse_args()
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    import era_boojum_amd as E
    from era_boojum_amd import field_np as F
    from era_boojum_amd import memcopy_format as M
    from era_boojum_amd import sha256_circuit as S
    assert F._NATIVE is not None, "libsynth_host.so is not built (python -m era_boojum_amd.build)"
    ctx = E.Context(0)
    t0 = time.time()
    c, info = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(args.log_n)), return_info=True)
    V, n, log_n = c.num_vars, 1 << c.log_n, c.log_n
    var_ids = np.ascontiguousarray(info["var_ids"], dtype=np.int32)
    print("circuit: %d x 2^%d cells, %d variables, synthesis %.1f s" % (V, log_n, info["num_variables"], time.time() - t0), flush=True)
    hint = np.where(var_ids >= 0, var_ids.astype(np.uint64), np.uint64(1 << 63))
    d_hint, d_sig = ctx.malloc(8 * V * n), ctx.malloc(8 * V * n)

    def device_path():
        t = time.perf_counter()
        ctx.h2d(d_hint, hint)
        ctx.sigmas_from_placement(d_hint, V, log_n, c.non_residues, d_sig)
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    def kernels_only():
        ctx.timer_start()
        ctx.sigmas_from_placement(d_hint, V, log_n, c.non_residues, d_sig)
        return ctx.timer_stop_ms()

    device_path()                                               # warm-up: scratch, twiddles, code objects
    assert np.array_equal(ctx.d2h(d_sig, (V, n)), c.sigmas), "device sigma differs from the circuit's"
    print("device sigma == circuit sigma (%d words)" % (V * n), flush=True)
    if args.operator_only:
        kernels_only()
        return
    res = {"log_n": log_n, "num_vars": V, "cells": V * n, "variables": int(info["num_variables"]), "sigma_equal": True}
    res["device_path_ms"], res["device_path_runs_ms"] = median3(device_path)
    res["device_kernels_ms"], res["device_kernels_runs_ms"] = median3(kernels_only)

    ident = np.empty_like(c.sigmas)                              # identities k_col * omega^row: where the host walk starts
    om = F.powers(F.omega(log_n), n)
    for col in range(V):
        ident[col] = F.mul(om, np.uint64(c.non_residues[col]))
    work = np.empty_like(ident)

    def host_path():
        work[:] = ident
        t = time.perf_counter()
        F._NATIVE.synth_sigma_from_placement(var_ids.ctypes.data, V, n, int(info["num_variables"]), work.ctypes.data)
        t_walk = time.perf_counter() - t
        ctx.h2d(d_sig, work)
        ctx.sync()
        host_path.walk_ms.append(t_walk * 1e3)
        return (time.perf_counter() - t) * 1e3
    host_path.walk_ms = []
    res["host_path_ms"], res["host_path_runs_ms"] = median3(host_path)
    res["host_walk_ms"] = statistics.median(host_path.walk_ms)
    assert np.array_equal(work, c.sigmas)
    ctx.free(d_hint)
    ctx.free(d_sig)
    del work, ident, hint

    # (c) a proof from all_values alone against a proof that brings the hint
    total = sum(t.shape[0] for t in S.sha_tables())
    wit = M.write_witness_vec([], info["all_values"], c.multiplicities[0, :total].astype(np.uint32))
    hint_dump = M.write_variables_hint(var_ids)
    setup = E.ProverSetup(ctx, c, 8, 16, 100, variables_hint_dump=hint_dump)
    lib = setup._lib

    def proof(with_hint):
        def run():
            h = C.c_void_p()
            t = time.perf_counter()
            ctx._check(lib.bj_prove_from_dumps(ctx._h, setup._h, wit, len(wit), hint_dump if with_hint else None,
                                               len(hint_dump) if with_hint else 0, None, 0, C.byref(h)))
            ms = (time.perf_counter() - t) * 1e3
            run.proofs.append(setup._finish(h)[0])
            return ms
        run.proofs = []
        return run
    a, b = proof(True), proof(False)
    a()                                                         # warm-up: the proof workspace
    res["prove_from_dumps_with_hint_ms"], res["prove_from_dumps_with_hint_runs_ms"] = median3(a)
    res["prove_from_dumps_without_hint_ms"], res["prove_from_dumps_without_hint_runs_ms"] = median3(b)
    assert all(np.array_equal(p, a.proofs[0]) for p in a.proofs + b.proofs), "proofs differ"
    res["proofs_identical"] = True
    res["setup_device_bytes"] = setup.device_bytes()
    setup.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
