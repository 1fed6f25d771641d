"""-m gpu: the copy-permutation polynomials built on the device from the variable placement (bj_sigmas_from_placement,
csrc/setup_placement.hip), the setup made from a placement (bj_setup_create_from_placement) and proofs from all_values alone
(bj_prove_from_dumps with no hint).  Everything is integer work: every comparison is exact.

The comparator is the project's own `sha256_circuit.sigma_from_placement`: its native walk (the serial loop of the reference's
create_permutation_polys, setup.rs:419-503) and its numpy restatement.  The first test runs both on one input, so the comparator
cannot drift; placements with indices up to 2^32 - 2 go through the numpy path only (the native walk indexes int32 tables of
num_vars entries)."""
import functools

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import field_np as F
from era_boojum_amd import memcopy_format as M
from era_boojum_amd import proof_format
from era_boojum_amd import sha256_circuit as S
from gpu_util import ctx

pytestmark = pytest.mark.gpu

PLACEHOLDER = np.uint64(1 << 63)
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)
MAX_INDEX = (1 << 32) - 2


def identities(V, log_n, ks):
    om = F.powers(F.omega(log_n), 1 << log_n)
    return np.stack([F.mul(om, np.uint64(k)) for k in ks[:V]])


def expected_sigmas(var_ids, log_n, ks, native):
    """sigma_from_placement on the identities; native=False forces the numpy path."""
    sig = identities(var_ids.shape[0], log_n, ks)
    saved = F._NATIVE
    if not native:
        F._NATIVE = None
    try:
        assert native is False or F._NATIVE is not None, "libsynth_host.so is not built"
        S.sigma_from_placement(var_ids, int(var_ids.max()) + 1, sig)
    finally:
        F._NATIVE = saved
    return sig


def make_placement(log_n, V, seed, sparse):
    """[V][n] int64, negative = placeholder.  Random variables used about three times each (some once, some never), 10 %
    placeholders; with V >= 3 one variable fills a whole column and one column holds placeholders only; with more than 2^21
    cells one variable sits in 40 % of all cells (> 2^20 of them, in every column); sparse: indices spread up to 2^32 - 2."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    cells = V * n
    k = max(4, cells // 3)
    v = rng.integers(0, k, size=(V, n), dtype=np.int64)
    v[rng.random((V, n)) < 0.10] = -1
    long_var, column_var = k, k + 1
    if cells > (1 << 21):
        v[rng.random((V, n)) < 0.40] = long_var
        assert int((v == long_var).sum()) > (1 << 20) and all((v[c] == long_var).any() for c in range(V))
    elif V >= 3:
        v[V // 2] = column_var
        v[V - 1] = -1
    counts = np.bincount(v[v >= 0])
    assert (counts == 1).any() and (counts > 2).any() and (v < 0).any()
    if sparse:   # a monotone map onto scattered indices: same permutation, keys in every radix digit
        top = int(v.max())
        pool = np.unique(rng.integers(0, MAX_INDEX, size=2 * (top + 1), dtype=np.int64))
        pool = pool[np.sort(rng.choice(len(pool), top + 1, replace=False))]
        pool[-1] = MAX_INDEX
        v = np.where(v >= 0, pool[np.maximum(v, 0)], -1)
        assert int(v.max()) == MAX_INDEX
    return v


def device_sigmas(var_ids, log_n, ks, pad_in=8, pad_out=24):
    V, n = var_ids.shape
    hint = np.full((V, n + pad_in), PLACEHOLDER, dtype=np.uint64)
    hint[:, :n] = np.where(var_ids >= 0, var_ids.astype(np.uint64), PLACEHOLDER)
    c = ctx()
    d_in = c.upload(hint)
    d_out = c.upload(np.full((V, n + pad_out), SENTINEL, dtype=np.uint64))
    try:
        c.sigmas_from_placement(d_in, V, log_n, ks, d_out, place_stride=n + pad_in, sig_stride=n + pad_out)
        got = c.d2h(d_out, (V, n + pad_out))
    finally:
        c.free(d_in)
        c.free(d_out)
    assert np.all(got[:, n:] == SENTINEL), "wrote between the columns"
    return got[:, :n]


def test_operator_equals_both_paths_of_the_comparator():
    log_n, V = 10, 3
    ks = S.non_residues(V, 1 << log_n)
    v = make_placement(log_n, V, seed=1, sparse=False)
    native, restated = expected_sigmas(v, log_n, ks, native=True), expected_sigmas(v, log_n, ks, native=False)
    assert np.array_equal(native, restated)
    assert not np.array_equal(native, identities(V, log_n, ks))
    assert np.array_equal(device_sigmas(v, log_n, ks), native)


@pytest.mark.parametrize("log_n,V", [(10, 1), (10, 92), (16, 3), (16, 92), (20, 1), (20, 3)])
def test_operator_on_sparse_placements(log_n, V):
    """Every log_n of {10, 16, 20} and every column count of {1, 3, 92}; (20, 3) holds the variable with more than 2^20 cells,
    whose run the scatter's search has to cross and whose order tests the stability of the sort."""
    ks = S.non_residues(V, 1 << log_n)
    v = make_placement(log_n, V, seed=100 * log_n + V, sparse=True)
    got = device_sigmas(v, log_n, ks)
    want = expected_sigmas(v, log_n, ks, native=False)
    assert np.array_equal(got, want)
    assert int(got.max()) < E.P


@functools.lru_cache(maxsize=None)
def sha_circuit(log_n):
    c, info = S.sha256_circuit(S.bench_message(S.message_len_for_log_n(log_n), seed=11), return_info=True)
    assert c.log_n == log_n
    return c, info


@pytest.mark.parametrize("log_n", [16, 20])
def test_real_circuit_sigmas(log_n):
    c, info = sha_circuit(log_n)
    got = device_sigmas(info["var_ids"], log_n, c.non_residues, pad_in=0, pad_out=0)
    assert np.array_equal(got, c.sigmas)


def test_setup_from_placement_is_the_setup_from_host_sigmas():
    from oracle import verifier as OV
    c, info = sha_circuit(16)
    n = 1 << c.log_n
    a = E.ProverSetup(ctx(), c, 8, 16, 30)
    b = E.ProverSetup.from_placement(ctx(), c, info["var_ids"], 8, 16, 30)
    try:
        assert np.array_equal(a.cap(), b.cap())
        assert b.device_bytes() == a.device_bytes() + 4 * c.num_vars * n
        d_vars, d_mult = ctx().upload(c.variables), ctx().upload(c.multiplicities)
        pa, _ = a.prove_dev(d_vars, d_mult)
        pb, _ = b.prove_dev(d_vars, d_mult)
        ctx().free(d_vars)
        ctx().free(d_mult)
        assert np.array_equal(pa, pb)
        total = sum(t.shape[0] for t in S.sha_tables())
        wit = M.write_witness_vec([(col, row) for col, row, _ in c.public_inputs], info["all_values"],
                                  c.multiplicities[0, :total].astype(np.uint32))
        with_hint, _ = b.prove_from_dumps(wit, M.write_variables_hint(info["var_ids"]))
        without, _ = b.prove_from_dumps(wit, None)
        assert np.array_equal(with_hint, without) and np.array_equal(without, pa)
        assert OV.verify(OV.VerificationKey(c, b.cap(), 8, 16), proof_format.parse(without, security_level=30))
    finally:
        a.close()
        b.close()


def test_refusals_carry_a_status_and_a_message():
    c, info = S.sha256_circuit(S.bench_message(100, seed=7), return_info=True)
    v = info["var_ids"]
    V, n = v.shape
    hint = M.write_variables_hint(v)

    def refuse(dump, match):
        with pytest.raises(E.BoojumHipError, match=match):
            E.ProverSetup(ctx(), c, 8, 16, 30, variables_hint_dump=dump)

    refuse(M.write_variables_hint(v[:-1]), "invalid.*%d columns, the circuit has %d" % (V - 1, V))
    refuse(hint[:-8], "invalid.*DenseVariablesCopyHint dump: truncated")
    refuse(M.write_variables_hint(v[:, :n // 2]), "invalid.*column 0 has %d cells, not %d" % (n // 2, n))
    beyond = v.astype(np.int64)
    beyond[3, 5] = MAX_INDEX + 1
    refuse(M.write_variables_hint(beyond), r"unsupported.*index above 2\^32 - 2")
    at_limit = v.astype(np.int64)              # 2^32 - 2 itself is a variable like any other
    at_limit[3, 5] = MAX_INDEX
    E.ProverSetup(ctx(), c, 8, 16, 30, variables_hint_dump=M.write_variables_hint(at_limit)).close()
    # the operator's own limits, refused before anything is read
    d = ctx().malloc(64)
    ks = [1] * 4096
    for V_, log_n_, match in ((1, 31, "log_n 31 > 30"), (4096, 20, r"num_vars \* n < 2\^32")):
        with pytest.raises(E.BoojumHipError, match="unsupported.*" + match):
            ctx().sigmas_from_placement(d, V_, log_n_, ks, d)
    ctx().free(d)
    # a setup made from host sigmas holds no placement: no hint is the null argument it has always been
    total = sum(t.shape[0] for t in S.sha_tables())
    wit = M.write_witness_vec([(col, row) for col, row, _ in c.public_inputs], info["all_values"],
                              c.multiplicities[0, :total].astype(np.uint32))
    a = E.ProverSetup(ctx(), c, 8, 16, 30)
    try:
        with pytest.raises(E.BoojumHipError, match="invalid.*bj_prove_from_dumps: null argument"):
            a.prove_from_dumps(wit, None)
    finally:
        a.close()
