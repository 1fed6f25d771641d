"""-m gpu: a plain `bench.py` run times the headline proofs and nothing else, and `--dump-outputs` writes the last timed proof
exactly as the library computes it for the same seeded circuit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import sha256_circuit as SHA
from gpu_util import ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_the_timed_proof(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TORCHELASTIC_RUN_ID", "BJ_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-n", "14", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "prover_constraints_per_sec" and out["unit"] == "rows/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u64" and out["steps"] == 3 and out["ms_per_step"] > 0
    assert abs(out["value"] - (1 << 14) / (out["ms_per_step"] / 1e3)) <= 0.01 * out["value"]
    # the secondary legs and the verifier check belong to --full
    assert not {"host_witness", "host_witness_pipelined", "ntt", "throughput_2_in_flight", "scale_replay", "cpu_baseline"} & set(out)
    assert "verified" not in out["config"]

    dumped = np.load(tmp_path / "out" / "proof.npy")
    assert dumped.dtype == np.float64 and dumped.shape == (out["config"]["proof_bytes"] // 8, 2)
    assert np.all(dumped == np.floor(dumped)) and dumped.min() >= 0 and dumped.max() < 2.0 ** 32
    words = dumped[:, 0].astype(np.uint64) | (dumped[:, 1].astype(np.uint64) << np.uint64(32))

    c = SHA.sha256_circuit(SHA.bench_message(SHA.message_len_for_log_n(14), seed=42))
    setup = E.ProverSetup(ctx(), c, 8, 16, 100, transcript="poseidon2")
    want, _ = setup.prove()
    setup.close()
    assert np.array_equal(words, want)
