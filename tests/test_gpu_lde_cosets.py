"""-m gpu: bj_lde_cosets_batch at 9 to 64 cosets, where a real NTT pass runs, against the CPU oracle (bit for bit, canonical residues;
tests/test_lde_coset_cases.py holds the oracle to the definition at these widths).  The coset count is an input of the kernels:
    ntt_first5 / ntt_first4 fill tws[] with n_cosets * 31 / * 15 entries, 256 per trip: the second trip starts at 9 / 18 cosets;
    launch_ntt_front10 issues one launch per eight cosets and the kernel divides its block index by the count of that launch;
    front10_table and round_scale write [n_cosets][1024] / [n_cosets][32] into regions of the context's small block that hold 64;
    pick_cols_per_block (csrc/ntt_plan.h) gives the strided and local passes more than one column per workgroup from 4096 workgroups on,
    which 64 cosets reach at 2^12..2^18 rows (tests/lde_coset_shapes.py, held to the header by tests/test_ntt_plan_host.py);
    bj::lde_cosets_strided bit-reverses the coset index over log_lde = 4, 5, 6 bits.
Columns as in test_gpu_ntt_w16_steps: random canonical words, all p - 1, words >= p.  Every output lies between guard words, which
come back untouched, and so does the input."""
import functools

import numpy as np
import pytest

import era_boojum_amd as E
import oracle as O
import lde_coset_shapes as shapes
from gpu_util import DevBuf, ctx, oracle_threads, P

pytestmark = pytest.mark.gpu

GUARD = 16                                  # words in front of and behind the output (128 bytes: the output keeps its alignment)
GUARD_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)


@functools.lru_cache(maxsize=2)
def _columns(log_n, n_cols):
    """Column c is of kind c % 3: random canonical words, all p - 1, words in [p, 2^64).  A single column takes kind i % 3 at row i."""
    n = 1 << log_n
    rng = np.random.default_rng(6400 + log_n)
    kinds = [lambda: rng.integers(0, P, size=n, dtype=np.uint64),
             lambda: np.full(n, P - 1, dtype=np.uint64),
             lambda: (np.uint64(P) + rng.integers(0, 2**32 - 1, size=n, dtype=np.uint64)).astype(np.uint64)]
    if n_cols == 1:
        three = np.stack([k() for k in kinds])
        out = three[np.arange(n) % 3, np.arange(n)][None, :]
    else:
        out = np.stack([kinds[c % 3]() for c in range(n_cols)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def _reference(log_n, n_cols, log_lde):
    """One oracle call per (size, columns, extension), shared by the cases that slice it; read-only."""
    want = O.lde_batch(_columns(log_n, n_cols), log_lde, threads=oracle_threads(16))
    want.setflags(write=False)
    return want


def _extend(mono, want, log_n, log_lde, begin, count, unaligned=False, call=None):
    """cosets [begin, begin + count) of the 2^log_lde-fold extension of `mono` (device input `call` reads, default the natural-order columns)
    == want[:, begin:begin + count, :]; guard words and input intact.  unaligned: input at an odd 8-byte address with column stride n + 1
    and output at an odd address, as test_gpu_ntt.test_lde_and_ntt_with_unaligned_buffers_and_odd_strides builds them."""
    n_cols, n = mono.shape
    assert n == 1 << log_n
    words = n_cols * count * n
    if unaligned:
        stride = n + 1
        src = np.random.default_rng(6500 + log_n).integers(0, 2**64 - 1, size=n_cols * stride + 1, dtype=np.uint64)      # the gaps: any words
        for c in range(n_cols):
            src[1 + c * stride: 1 + c * stride + n] = mono[c]
    else:
        stride, src = n, mono
    lead = GUARD + (1 if unaligned else 0)
    d_in = DevBuf(src)
    d_out = DevBuf(np.full(lead + words + GUARD, GUARD_WORD, dtype=np.uint64))
    try:
        in_ptr = d_in.ptr + (8 if unaligned else 0)
        if call is None:
            ctx().lde_cosets_batch(in_ptr, d_out.ptr + 8 * lead, log_n, n_cols, log_lde, begin, count, col_stride=stride)
        else:
            call(in_ptr, d_out.ptr + 8 * lead)
        got = d_out.get()
        src_after = d_in.get(src.shape)
    finally:
        d_in.free(); d_out.free()
    assert (got[:lead] == GUARD_WORD).all() and (got[lead + words:] == GUARD_WORD).all()
    assert np.array_equal(src_after, src)
    got = got[lead:lead + words].reshape(n_cols, count, n)
    if not np.array_equal(got, want[:, begin:begin + count, :]):
        bad = np.argwhere((got != want[:, begin:begin + count, :]).any(axis=2))
        raise AssertionError("(column, coset - begin) that differ, first of %d: %s" % (len(bad), bad[:8].tolist()))


# log_n, unaligned, (log_lde, begin, count): the smallest size that reaches each pass of csrc/ntt_plan.h
SMALL = [
    (0, False, (6, 0, 64)),                                                              # canonicalising copy
    (5, False, (4, 0, 16)), (5, False, (6, 37, 27)), (11, False, (4, 0, 16)), (11, False, (6, 37, 27)),      # G
    (12, False, (4, 0, 16)), (12, False, (5, 3, 19)),                                     # L12
    (13, False, (4, 0, 16)), (13, False, (6, 0, 64)),                                     # R1 L12
    (14, False, (5, 0, 17)), (14, False, (5, 0, 18)), (14, False, (6, 0, 64)), (14, False, (6, 37, 27)),     # F4 L10
    (14, True, (4, 0, 8)), (14, True, (4, 0, 9)), (14, True, (6, 0, 64)),                  # F5 L9
    (15, False, (4, 3, 9)), (15, False, (6, 0, 64)),                                      # F5 L10
    (16, False, (4, 0, 16)),                                                             # S4 L12
    (17, False, (6, 0, 64)),                                                             # R1 S4 L12
]


@pytest.mark.parametrize("log_n,unaligned,cosets", SMALL, ids=["2p%d%s-lde%d-from%d-count%d" % (l, "u" if u else "", c[0], c[1], c[2]) for l, u, c in SMALL])
def test_wide_lde_at_the_smallest_size_of_each_pass(log_n, unaligned, cosets):
    """Three columns.  The counts are chosen at the edges of the twiddle fills at the head of the front passes, 256 entries per trip
    of the fill loop:
        ntt_first5 (2^14 unaligned, 2^15): 31 entries per coset: 8 cosets = 248 entries, the last single-trip fill; 9 cosets = 279,
            the first that needs a second trip; 64 cosets fill tws[64 * 40] to its last used word;
        ntt_first4 (2^14 aligned): 15 entries per coset: 17 cosets = 255 entries, the last single-trip fill; 18 = 270, the first
            two-trip fill; 64 cosets fill tws[64 * 16].
    (6, 37, 27) is a range that starts at an odd coset and has a count that is no power of two; 64 cosets write the round scales and,
    at 2^22 only, the front table to the ends of their regions."""
    log_lde, begin, count = cosets
    mono = _columns(log_n, 3)
    _extend(mono, _reference(log_n, 3, log_lde), log_n, log_lde, begin, count, unaligned=unaligned)


@pytest.mark.parametrize("case", shapes.MULTI_COLUMN, ids=[shapes.multi_column_line(c).replace(" ", "-").replace('"', "") for c in shapes.MULTI_COLUMN])
def test_several_columns_per_workgroup(case):
    """64 cosets put 4096 workgroups behind few columns, so pick_cols_per_block hands a workgroup of ntt_local12<., 12 / 10 / 9> and
    ntt_strided4 several columns through one LDS tile (col1 = min(col0 + cpb, n_cols)); with at most eight cosets that took 2^20 rows
    and more, where only S8, L12 and L9 were reached.  cols_per_block of every row (tests/ntt_plan_check.cpp asserts them against
    csrc/ntt_plan.h):
        2^12 x 127 columns: 2, the last workgroup with one column (L12)
        2^18 x 3 columns, aligned: 8, the three columns in one workgroup (F4, S4, L10); unaligned: 8 (F5, S4, L9)
        2^17 x 3 columns: 2, workgroups of two columns and of one (R1, S4, L12)"""
    log_n, n_cols = case["log_n"], case["n_cols"]
    assert case["n_cosets"] == 64
    mono = _columns(log_n, n_cols)
    _extend(mono, _reference(log_n, n_cols, 6), log_n, 6, 0, 64, unaligned=not case["aligned"])


def _tiled_index(e):
    """The tiled layout of a 2^22-word column (include/boojum_hip.h, csrc/tiled_layout.h: tiled_index)."""
    e = np.asarray(e, dtype=np.int64)
    return ((e >> 3) & 511) * 8192 + ((e >> 1) & 3) * 2048 + (e >> 12) * 2 + (e & 1)


@pytest.mark.parametrize("case", shapes.FRONT10, ids=[shapes.front10_line(c).replace(" ", "-") for c in shapes.FRONT10])
def test_two_pass_plan_at_2p22_with_short_and_second_launches(case):
    """2^22 is the only size with ntt_front10, which runs at most eight cosets per launch and decodes coset = (block >> 3 or 4) % cosets
    of that launch.  One column.  Natural-order monomials: cosets [1, 4) of 4, one launch of three (a count that is no power of two);
    cosets [3, 12) of 16, launches of 8 + 1 (the second launch reads the table and writes the output 8 cosets further on).  Tiled
    monomials (bj_lde_cosets_batch_tiled): cosets [5, 16) of 16, launches of 8 + 3."""
    log_n, n = 22, 1 << 22
    assert ctx().monomials_tiled(22)
    log_lde, begin, count = case["log_lde"], case["begin"], case["count"]
    mono = _columns(log_n, 1)
    want = _reference(log_n, 1, log_lde)
    if not case["tiled"]:
        _extend(mono, want, log_n, log_lde, begin, count)
        return
    tiled = np.empty_like(mono)
    tiled[:, _tiled_index(np.arange(n))] = mono
    _extend(tiled, want, log_n, log_lde, begin, count,
            call=lambda d_in, d_out: ctx().lde_cosets_batch_tiled(d_in, d_out, log_n, 1, log_lde, begin, count))


def test_trace_to_lde_at_sixteen_cosets():
    """bj_trace_to_lde_batch at 2^12 x 16: the extension, and the monomials left in the input."""
    log_n, log_lde, n_cols = 12, 4, 3
    trace = _columns(log_n, n_cols)
    mono = O.ifft_batch(trace, 1, threads=4)
    want = O.lde_batch(mono, log_lde, threads=4)
    d_t = DevBuf(trace)
    d_o = DevBuf(np.full(2 * GUARD + want.size, GUARD_WORD, dtype=np.uint64))
    ctx().trace_to_lde_batch(d_t.ptr, d_o.ptr + 8 * GUARD, log_n, n_cols, log_lde)
    got, left = d_o.get(), d_t.get(trace.shape)
    d_t.free(); d_o.free()
    assert np.array_equal(got[GUARD:-GUARD].reshape(want.shape), want)
    assert (got[:GUARD] == GUARD_WORD).all() and (got[-GUARD:] == GUARD_WORD).all()
    assert np.array_equal(left, mono)


@pytest.mark.parametrize("log_n,log_lde,begin,count", [(5, 7, 0, 1), (5, 6, 64, 1), (5, 6, 37, 28), (5, 4, 3, 14), (27, 6, 0, 1)],
                         ids=["log_lde-7", "begin-is-L", "count-one-past-L", "count-one-past-L-of-16", "domain-past-2p32"])
def test_refused_coset_ranges_write_nothing_and_leave_the_context_working(log_n, log_lde, begin, count):
    """log_lde = 7; begin = L; count = L - begin + 1; log_n + log_lde > 32 (bj_lde_cosets_batch checks its arguments before it touches
    the device: no word of a 2^27-row column exists here).  Each is reported, nothing is written, and the same context then computes a
    correct 16-coset extension."""
    d_in = DevBuf(_columns(5, 3))
    d_out = DevBuf(np.full(128 * 32, GUARD_WORD, dtype=np.uint64))
    with pytest.raises(E.BoojumHipError):
        ctx().lde_cosets_batch(d_in.ptr, d_out.ptr, log_n, 1, log_lde, begin, count)
    untouched = d_out.get()
    d_in.free(); d_out.free()
    assert (untouched == GUARD_WORD).all()
    _extend(_columns(5, 3), _reference(5, 3, 4), 5, 4, 0, 16)
