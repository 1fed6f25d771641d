"""-m gpu: the factored radix-16 steps of csrc/ntt_r16.hip (x[m] *= beta^m, then a DFT-16 by signed powers of two) against the CPU
oracle, at the smallest size that reaches each pass kernel and step shape of csrc/ntt_plan.h:
    2^12  L12: ntt_local12 alone (three full steps);     2^14  F4 L10: ntt_first4 and the two-round partial step (four DFT-4)
    2^15  F5 L10, and through odd addresses 2^14 F5 L9: the one-round partial step, which keeps generic butterflies
    2^16  S4 L12: ntt_strided4;     2^20  S8 L12: ntt_strided8
    2^22  F10 L12: ntt_front10 forward over 8 cosets from tiled monomials; the inverse (natural-order ntt_front10, the inverse root)
          into tiled monomials through ntt_local12_pair_tiled
Forward on the unit shift (no per-round scales: the steps whose beta is 1 run no product at all) and on the LDE cosets 7 omega^bitrev(c)
for c = 5, 6; the inverse of the forward transform is the input.  Columns: random canonical words, all p - 1 (every product and sum
at the top of the range), and non-canonical words >= p (the entry points admit any u64).  One oracle call per size, shared."""
import numpy as np
import pytest

import oracle as O
from gpu_util import DevBuf, ctx, P

pytestmark = pytest.mark.gpu


def _columns(log_n, seed):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    canon = rng.integers(0, P, size=n, dtype=np.uint64)
    top = np.full(n, P - 1, dtype=np.uint64)
    weak = (np.uint64(P) + rng.integers(0, 2**32 - 1, size=n, dtype=np.uint64)).astype(np.uint64)      # p .. 2^64 - 1
    return np.stack([canon, top, weak])


@pytest.fixture(scope="module", params=[12, 14, 15, 16, 20])
def case(request):
    log_n = request.param
    mono = _columns(log_n, 1600 + log_n)
    return log_n, mono, O.fft_batch(mono, 1, threads=8), O.lde_batch(mono, 3, threads=8)


def test_forward_unit_shift(case):
    log_n, mono, want, _ = case
    d_in, d_out = DevBuf(mono), DevBuf(nelems=mono.size)
    ctx().ntt_forward_batch(d_in.ptr, d_out.ptr, log_n, 3)
    got = d_out.get(mono.shape)
    d_in.free(); d_out.free()
    assert np.array_equal(got, want)


def test_forward_two_lde_cosets(case):
    log_n, mono, _, lde = case
    d_in, d_out = DevBuf(mono), DevBuf(nelems=2 * mono.size)
    ctx().lde_cosets_batch(d_in.ptr, d_out.ptr, log_n, 3, 3, 5, 2)          # cosets 5 and 6 of 8: shifts 7 omega^bitrev(c)
    got = d_out.get((3, 2, 1 << log_n))
    d_in.free(); d_out.free()
    assert np.array_equal(got, lde[:, 5:7, :])


@pytest.mark.parametrize("coset", [1, 7])
def test_inverse_of_forward_is_the_input(case, coset):
    log_n, mono, want, lde = case
    vals = want if coset == 1 else np.ascontiguousarray(lde[:, 0, :])      # LDE coset 0 = the transform on shift 7
    d = DevBuf(vals)
    ctx().bitreverse_batch(d.ptr, d.ptr, log_n, 3)
    ctx().intt_batch(d.ptr, d.ptr, log_n, 3, coset=coset)
    got = d.get(mono.shape)
    d.free()
    assert np.array_equal(got, O.canonical(mono))


def test_unaligned_columns_take_first5_and_the_nine_round_local_pass():
    log_n, n = 14, 1 << 14
    mono = _columns(log_n, 1614)
    buf = np.zeros(3 * (n + 1) + 1, dtype=np.uint64)
    for c in range(3):
        buf[1 + c * (n + 1): 1 + c * (n + 1) + n] = mono[c]
    d = DevBuf(buf)
    ctx().ntt_forward_batch(d.ptr + 8, d.ptr + 8, log_n, 3, col_stride=n + 1, coset=7)
    got = d.get(buf.shape)
    d.free()
    want = O.fft_batch(mono, 7, threads=8)
    for c in range(3):
        assert np.array_equal(got[1 + c * (n + 1): 1 + c * (n + 1) + n], want[c])


def _tiled_index(e):
    e = np.asarray(e, dtype=np.int64)
    return ((e >> 3) & 511) * 8192 + ((e >> 1) & 3) * 2048 + (e >> 12) * 2 + (e & 1)


@pytest.mark.parametrize("which", ["random and non-canonical", "all p - 1"])
def test_two_pass_plan_at_2_22(which):
    """values -> tiled monomials (inverse ntt_front10 + ntt_local12_pair_tiled) -> 8 cosets (tiled ntt_front10 + ntt_local12), 1-2 columns"""
    log_n, n = 22, 1 << 22
    cols = _columns(log_n, 1622)
    vals = np.ascontiguousarray(cols[[0, 2]] if which.startswith("random") else cols[[1]])
    k = vals.shape[0]
    mono = O.ifft_batch(vals, 1, threads=32)
    want = O.lde_batch(mono, 3, threads=32)
    tiled = np.empty_like(mono)
    tiled[:, _tiled_index(np.arange(n))] = mono
    d_v, d_o = DevBuf(vals), DevBuf(nelems=want.size)
    ctx().intt_batch_tiled(d_v.ptr, d_v.ptr, log_n, k)
    got_mono = d_v.get(vals.shape)
    ctx().lde_cosets_batch_tiled(d_v.ptr, d_o.ptr, log_n, k, 3, 0, 8)
    got = d_o.get(want.shape)
    # the forward transform of the unit shift from natural-order monomials (ntt_front10's natural variant without scales), and back
    d_n = DevBuf(mono)
    ctx().ntt_forward_batch(d_n.ptr, d_n.ptr, log_n, k)
    ctx().bitreverse_batch(d_n.ptr, d_n.ptr, log_n, k)
    back = d_n.get(vals.shape)
    for d in (d_v, d_o, d_n):
        d.free()
    assert np.array_equal(got_mono, tiled)
    assert np.array_equal(got, want)
    assert np.array_equal(back, O.canonical(vals))
