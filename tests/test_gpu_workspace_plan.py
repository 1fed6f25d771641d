"""-m gpu: a proof takes exactly the workspace its plan holds (csrc/workspace_plan.h).

Every case proves on a context of its own, so that the context has learned no high-water mark and the reservation is the plan's
total.  The proof must be the oracle's, need no overflow slab and stay inside the reservation, and what it leaves unused must fit
in the plan's allowances plus the 64-word alignment of every entry: an exact entry that is never taken, or planned too large,
breaks that bound.  The bound comes from the plan itself through the host helper library (csrc/witness_plan_shim.cpp).  The
high-water marks are those of the prover before it had a plan (tests/golden/workspace_high_water.json, recorded with that prover's
library by tools/workspace_record.py): the order and the sizes of the buffers have not changed."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, build, proof_format, synthetic as S
from gpu_util import ctx as session_ctx
from oracle import prover as OP
from test_gpu_prover import _compare

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "workspace_high_water.json")
FRI_LDE, CAP, SEC = 8, 16, 30
HOST_NONE, HOST_ABSORBING, HOST_NOT_ABSORBING = 0, 1, 2
# name: (circuit, entry point, what it is given)
CASES = {
    "sha256_2p14_resident": ("sha14", "dev", {}),
    "lookup_2p11_resident": ("lookup11", "dev", {}),
    "lookup_2p11_resident_counted": ("lookup11", "dev", {"count": True}),
    "lookup_2p11_host_absorbing": ("lookup11", "host", {}),
    "lookup_2p11_host_not_absorbing": ("lookup11", "host", {"no_absorb": True}),
    "recursion_2p10_resident": ("rec10", "dev", {}),
    "recursion_2p10_host_absorbing": ("rec10", "host", {}),
    "lookup_2p10_two_ranks": ("lookup10", "sharded", {}),
}
_circuits, _oracle = {}, {}


def circuit(name):
    if name not in _circuits:
        if name == "sha14":
            from era_boojum_amd import sha256_circuit as SHA
            _circuits[name] = SHA.sha256_circuit(SHA.bench_message(100, seed=7))
        elif name == "rec10":
            _circuits[name] = S.recursion_like_circuit(10, seed=7)
        else:   # lookup10: the circuit tests/sharded_worker.py builds for log_n 10
            _circuits[name] = S.sha_shaped_circuit(int(name[6:]), seed=7, table_bits=2)
    return _circuits[name]


def oracle_proof(name):
    if name not in _oracle:
        c = circuit(name)
        _oracle[name] = OP.prove(c, OP.Setup(c, FRI_LDE, CAP, threads=8), FRI_LDE, CAP, security_level=SEC, threads=8)
    return _oracle[name]


def prove(case, tmp_path):
    """[(proof words, bj_proof_workspace_bytes of that proof)], one per rank, each from a context that has proved nothing before."""
    cname, entry, opt = CASES[case]
    c = circuit(cname)
    if entry == "sharded":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
               str(_free_port()), os.path.join(HERE, "sharded_worker.py"), str(tmp_path), str(c.log_n), str(FRI_LDE), str(CAP), str(SEC)]
        r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return [(np.load(os.path.join(str(tmp_path), "proof_%d.npy" % k)), json.load(open(os.path.join(str(tmp_path), "workspace_%d.json" % k))))
                for k in range(2)]
    lib = E.load_library()
    session_ctx()
    ctx = E.Context(0)
    setup = E.ProverSetup(ctx, c, FRI_LDE, CAP, SEC)
    try:
        if entry == "dev":
            d_vars, d_mult = ctx.upload(c.variables), ctx.upload(c.multiplicities)
            buf, _ = setup.prove_dev(d_vars, d_mult, count_multiplicities=bool(opt.get("count")))
            ctx.free(d_vars)
            ctx.free(d_mult)
        else:
            if opt.get("no_absorb"):
                os.environ["BJ_PROVE_NO_ABSORB"] = "1"
                lib.bj_env_reload()
            try:
                buf, _ = setup.prove()
            finally:
                if os.environ.pop("BJ_PROVE_NO_ABSORB", None):
                    lib.bj_env_reload()
        return [(buf, dict(setup.last_workspace))]
    finally:
        setup.close()
        ctx.close()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def plan_summary(case, alpha_terms=1):
    """(total, allowance, entries, exact) of the plan of one rank of `case`, in words / entries.  alpha_terms: the powers of the
    quotient challenge, which the total and the exact words depend on and the other two do not."""
    cname, entry, opt = CASES[case]
    c = circuit(cname)
    lib = C.CDLL(build.build_canon_helper())
    lib.bj_workspace_plan_summary.restype = None
    new_pow, nq, sched, _ = B.fri_schedule(SEC, CAP, 0, FRI_LDE.bit_length() - 1, c.log_n)
    u = lambda xs: (C.c_uint * max(len(xs), 1))(*xs)
    nine = [c.log_n, c.num_vars, c.num_gp_vars, int(getattr(c, "num_witness_cols", 0)), c.num_constant_cols, c.lookup_width, c.lookup_reps,
            c.table_id_col, c.quotient_degree]
    absorbing = HOST_NOT_ABSORBING if opt.get("no_absorb") else HOST_ABSORBING   # the setups here hash with Poseidon2
    flags = [0, int(bool(opt.get("count")) and entry == "dev" and c.lookup_reps > 0), absorbing if entry == "host" else HOST_NONE, int(new_pow != 0)]
    out = (C.c_size_t * 4)()
    lib.bj_workspace_plan_summary(u(nine), C.c_uint(FRI_LDE), C.c_uint(CAP), C.c_uint(2 if entry == "sharded" else 1), C.c_uint(alpha_terms),
                                  u([p[0] for p in c.public_inputs]), u([p[1] for p in c.public_inputs]), C.c_size_t(len(c.public_inputs)),
                                  u(flags), (C.c_uint32 * 32)(*sched), C.c_size_t(len(sched)), C.c_size_t(nq), out)
    return tuple(int(x) for x in out)


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_proof_takes_the_workspace_of_its_plan(case, tmp_path):
    session_ctx()   # before anything loads the library: the session's context brings the HIP runtime up in the order torch needs
    want = oracle_proof(CASES[case][0])
    recorded = json.load(open(GOLDEN))[case]
    _, allowance, entries, _ = plan_summary(case)
    ranks = prove(case, tmp_path)
    assert len(ranks) == len(recorded)
    for (buf, ws), high_water_before in zip(ranks, recorded):
        _compare(proof_format.parse(buf, security_level=SEC), want)
        unused = ws["reserved_bytes"] - ws["high_water_bytes"]
        print("%s: reserved %d, high water %d (before the plan: %d), unused %d, bound %d = 8 * (%d allowance words + 64 * %d entries)"
              % (case, ws["reserved_bytes"], ws["high_water_bytes"], high_water_before, unused, 8 * (allowance + 64 * entries), allowance, entries))
        assert ws["overflow_slabs"] == 0
        assert ws["high_water_bytes"] <= ws["reserved_bytes"]
        assert unused <= 8 * (allowance + 64 * entries)
        assert ws["high_water_bytes"] == high_water_before
