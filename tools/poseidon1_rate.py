#!/usr/bin/env python3
"""Poseidon (v1) tree hasher (BJ_HASHER_POSEIDON, csrc/poseidon1.hip) against Poseidon2 on one MI355X, the two arms interleaved
in one process after a warm-up; medians and spreads:
  (a) the witness-tree leaf kernel at the bench geometry, 2^25 leaves x 93 columns (tree build minus its node layers);
  (b) the node layers of that tree (bj_merkle_tree_nodes);
  (c) the 2^22-row real SHA-256 proof, witness resident (bj_prove_dev): v1 trees + v1 transcript (the reference's
      run_sha256_prover_recursive_mode) against Poseidon2 trees + Poseidon2 transcript; the last v1 proof is checked by the
      oracle verifier with the v1 hashing layer of tests/poseidon1_layer.py.
Prints one JSON object (and writes it to --out).  --no-proof skips (c).
    python tools/poseidon1_rate.py [--reps 5] [--no-proof] [--out FILE]
Derived figures: HBM fraction by algorithmic bytes (8 W + 32 per leaf) at 8 TB/s; cycles per wave64 VALU instruction per SIMD
from the leaf time at the nominal 2.4 GHz over 256 CUs x 4 SIMDs (VALU instructions per permutation from the ISA)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import era_boojum_amd as E

P2, V1 = E.binding.HASHER_KINDS["poseidon2"], E.binding.HASHER_KINDS["poseidon"]      # BJ_HASHER_*
VALU_PER_PERM = {P2: 8588, V1: 20988}      # Poseidon2 (generated stream), v1 (poseidon1.hip): counted in the gfx950 ISA
NAMES = {P2: "poseidon2", V1: "poseidon"}


def _stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def trees(ctx, reps, log_leaves=25, width=93, cap=16):
    dev = torch.device("cuda", 0)
    leaves = 1 << log_leaves
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cols = torch.randint(-2**63, 2**63 - 1, (width, leaves), dtype=torch.int64, device=dev, generator=g)
    tree = torch.empty((ctx.merkle_tree_digests(leaves, cap), 4), dtype=torch.int64, device=dev)
    res = {h: {"build": [], "nodes": []} for h in NAMES}

    def one(h):
        ctx.set_tree_hasher(h)
        ctx.timer_start()
        ctx.merkle_tree_build(cols.data_ptr(), leaves, width, leaves, cap, tree.data_ptr())
        b = ctx.timer_stop_ms()
        ctx.timer_start()
        ctx.merkle_tree_nodes(tree.data_ptr(), leaves, cap)
        return b, ctx.timer_stop_ms()

    for h in NAMES:              # warm-up
        one(h)
    for _ in range(reps):
        for h in NAMES:
            b, n = one(h)
            res[h]["build"].append(b)
            res[h]["nodes"].append(n)
    ctx.set_tree_hasher(P2)
    out = {}
    perms_per_leaf = (width + 7) // 8
    for h, name in NAMES.items():
        leaf = [b - n for b, n in zip(res[h]["build"], res[h]["nodes"])]
        ms = statistics.median(leaf)
        bytes_alg = (8 * width + 32) * leaves
        valu_waves = perms_per_leaf * VALU_PER_PERM[h] * leaves / 64
        out[name] = {"leaf_ms": _stats(leaf), "node_layers_ms": _stats(res[h]["nodes"]),
                     "hbm_fraction_algorithmic": round(bytes_alg / (ms * 1e-3) / 8e12, 4),
                     "valu_per_permutation": VALU_PER_PERM[h],
                     "cycles_per_valu_nominal_clock": round(ms * 1e-3 * 2.4e9 * 256 * 4 / valu_waves, 2)}
    out["leaf_ratio_v1_over_p2"] = round(out["poseidon"]["leaf_ms"]["median"] / out["poseidon2"]["leaf_ms"]["median"], 3)
    out["node_ratio_v1_over_p2"] = round(out["poseidon"]["node_layers_ms"]["median"] / out["poseidon2"]["node_layers_ms"]["median"], 3)
    out["geometry"] = {"leaves": leaves, "columns": width, "cap": cap}
    del cols, tree
    torch.cuda.empty_cache()
    return out


def proofs(ctx, reps):
    from era_boojum_amd import proof_format, sha256_circuit as SHA
    t0 = time.perf_counter()
    c = SHA.sha256_circuit(SHA.bench_message(SHA.message_len_for_log_n(22)))
    synth_s = time.perf_counter() - t0
    dev = torch.device("cuda", 0)
    d_v = torch.from_numpy(np.ascontiguousarray(c.variables).view(np.int64)).to(dev)
    d_m = torch.from_numpy(np.ascontiguousarray(c.multiplicities).view(np.int64)).to(dev)
    setups = {P2: E.ProverSetup(ctx, c, 8, 16, 100, transcript="poseidon2"),
              V1: E.ProverSetup(ctx, c, 8, 16, 100, transcript="poseidon", tree_hasher="poseidon")}
    times = {h: [] for h in setups}
    last = None
    for h, s in setups.items():   # warm-up
        s.prove_dev(d_v.data_ptr(), d_m.data_ptr())
    for _ in range(reps):
        for h, s in setups.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            buf, _ = s.prove_dev(d_v.data_ptr(), d_m.data_ptr())
            times[h].append((time.perf_counter() - t) * 1e3)
            if h == V1:
                last = buf.copy()
    import poseidon1_layer as PL
    from oracle import prover as OP
    from oracle import verifier as OV
    layer = PL.poseidon1_layer()
    OP.hashing_layer = lambda hasher: layer
    ok = bool(OV.verify(OV.VerificationKey(c, setups[V1].cap(), 8, 16), proof_format.parse(last, security_level=100), transcript_kind=setups[V1].transcript_kind))
    n = 1 << c.log_n
    out = {"log_n": c.log_n, "synthesis_s": round(synth_s, 1), "v1_proof_verified": ok}
    for h, name in NAMES.items():
        ms = statistics.median(times[h])
        out[name] = {"proof_ms": _stats(times[h]), "rows_per_s": round(n / (ms * 1e-3))}
    out["ratio_v1_over_p2"] = round(out["poseidon"]["proof_ms"]["median"] / out["poseidon2"]["proof_ms"]["median"], 3)
    for s in setups.values():
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-proof", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = E.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"trees": trees(ctx, a.reps)}
    if not a.no_proof:
        out["proof_2p22_sha256"] = proofs(ctx, a.reps)
    ctx.release_workspace()
    txt = json.dumps(out)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
