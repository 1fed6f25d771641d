#!/usr/bin/env python3
"""bj_verify next to the proof it checks, on one box in one process.

    python tools/verify_rate.py [--shapes sha16,sha20,rec16] [--out profiles/verify_rate.json]

Shapes: sha16 / sha20 — the SHA-256 circuit at 2^16 / 2^20 rows with the bench parameters (fri_lde_factor 8, cap 16, security
100); rec16 — the recursion-class circuit at 2^16 rows with the golden proof's config (fri_lde_factor 2, cap 16, security 100:
100 queries).  Per shape, median of 5: the whole bj_verify call (wall clock around the synchronous call: upload of the query
section, host replay, both kernels, status read-back), its two kernels alone (HIP events, bj_verify_kernel_ms), and bj_prove_dev of
the same witness (median of 3).

    python tools/verify_rate.py --batch 1,8,64,512 [--shapes sha12,sha16]

adds the batch leg: per N, bj_verify_batch over N copies-with-distinct-buffers of the proof next to N looped bj_verify calls on the
same buffers, alternating the two for 5 rounds after one warm-up of each (proofs/s from the median wall time), and the four
phase times of bj_verify_batch_ms of the median batch.  `--batch N` with one number is the same for that N alone.

`--transcript` / `--tree-hasher` go to ProverSetup (default: Poseidon2 for both) and into every result row, e.g. `--transcript
poseidon --tree-hasher poseidon` for Poseidon (v1) trees, `--transcript keccak256` for Keccak ones."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sha16,sha20,rec16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", default=None, help="comma-separated batch sizes for the bj_verify_batch leg, e.g. 1,8,64,512")
    ap.add_argument("--transcript", default="poseidon2", choices=["poseidon2", "poseidon", "blake2s", "keccak256"])
    ap.add_argument("--tree-hasher", default=None, choices=["poseidon2", "poseidon", "blake2s", "keccak256"],
                    help="default: the transcript's usual hasher")
    args = ap.parse_args()
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    import numpy as np
    import era_boojum_amd as E
    from era_boojum_amd import sha256_circuit as SHA, synthetic as S
    ctx = E.Context(0)
    results = []
    for shape in args.shapes.split(","):
        if shape.startswith("sha"):
            log_n = int(shape[3:])
            c = SHA.sha256_circuit(SHA.bench_message(SHA.message_len_for_log_n(log_n)))
            cfg = (8, 16, 100)
        else:
            log_n = int(shape[3:])
            c = S.recursion_like_circuit(log_n, seed=3)
            cfg = (2, 16, 100)
        setup = E.ProverSetup(ctx, c, *cfg, transcript=args.transcript, tree_hasher=args.tree_hasher)
        v = np.ascontiguousarray(c.variables, dtype=np.uint64)
        if setup.num_witness_cols:
            v = np.ascontiguousarray(np.concatenate([v, c.witness], axis=0))
        d_v, d_m = ctx.upload(v), ctx.upload(np.ascontiguousarray(c.multiplicities, dtype=np.uint64))
        buf, _ = setup.prove_dev(d_v, d_m)          # first proof: the workspace reservation
        prove = []
        for _ in range(3):
            ctx.sync()
            t = time.perf_counter()
            buf, _ = setup.prove_dev(d_v, d_m)
            prove.append((time.perf_counter() - t) * 1e3)
        vk = setup.verifier()
        assert vk.verify(ctx, buf), "the proof does not verify"      # first call: scratch and twiddles
        whole, k_open, k_deep = [], [], []
        for _ in range(5):
            ctx.sync()
            t = time.perf_counter()
            r = vk.verify(ctx, buf)
            whole.append((time.perf_counter() - t) * 1e3)
            assert r
            a, b = vk.kernel_ms(ctx)
            k_open.append(a)
            k_deep.append(b)
        res = {"shape": shape, "transcript": args.transcript, "tree_hasher": args.tree_hasher, "log_n": c.log_n, "num_vars": c.num_vars, "fri_lde_factor": cfg[0], "cap_size": cfg[1], "security_level": cfg[2],
               "queries": int(buf[9]), "proof_words": int(buf.size), "verify_ms": statistics.median(whole), "verify_runs_ms": whole,
               "verify_openings_kernel_ms": statistics.median(k_open), "verify_deep_fri_kernel_ms": statistics.median(k_deep),
               "prove_dev_ms": statistics.median(prove), "prove_dev_runs_ms": prove,
               "verify_over_prove": statistics.median(whole) / statistics.median(prove)}
        if args.batch:
            res["batch"] = []
            for n in [int(x) for x in args.batch.split(",")]:
                proofs = [np.array(buf, copy=True) for _ in range(n)]      # N buffers: nothing is served from one cached copy
                assert all(vk.verify_batch(ctx, proofs)) and all(vk.verify(ctx, p) for p in proofs)      # warm-up of both, and the verdicts
                loop_ms, batch_ms, phases = [], [], []
                for _ in range(5):
                    ctx.sync()
                    t = time.perf_counter()
                    for p in proofs:
                        vk.verify(ctx, p)
                    loop_ms.append((time.perf_counter() - t) * 1e3)
                    ctx.sync()
                    t = time.perf_counter()
                    vk.verify_batch(ctx, proofs)
                    batch_ms.append((time.perf_counter() - t) * 1e3)
                    phases.append(vk.batch_ms(ctx))
                lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
                ph = phases[batch_ms.index(sorted(batch_ms)[2])]
                row = {"n": n, "loop_ms": lm, "batch_ms": bm, "loop_proofs_per_s": n / lm * 1e3, "batch_proofs_per_s": n / bm * 1e3,
                       "loop_runs_ms": loop_ms, "batch_runs_ms": batch_ms, "host_ms": ph[0], "upload_ms": ph[1], "openings_ms": ph[2],
                       "deep_fri_ms": ph[3]}
                print("  batch", json.dumps(row), flush=True)
                res["batch"].append(row)
        print(json.dumps(res), flush=True)
        results.append(res)
        vk.close()
        ctx.free(d_v)
        ctx.free(d_m)
        setup.close()
        ctx.release_workspace()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
