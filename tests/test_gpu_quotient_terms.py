"""-m gpu: bj_quotient_gates, bj_quotient_lookup, bj_quotient_copy_perm and bj_lookup_polys against tests/quotient_ref.py (the
operators restated from their definitions in python integers; tests/test_quotient_ref.py pins it on the oracle) on columns no
circuit produces: random uint64 words, a quarter of them in [p, 2^64), the words 0, 1, p-1, p, p+1, 2^32-1, 2^32, 2^64-2^32,
2^64-1 planted on lone lanes and across whole waves (quotient_cases.raw_columns), challenges canonical and in [p, 2^64),
outputs that start as arbitrary words wherever a kernel accumulates, column strides above the point count with the words
behind the points checked untouched.  tests/test_gpu_stage_ops.py runs the same operators on the oracle's LDEs of satisfied
circuits (one gate list, lookup widths 3 and 4, z = 1 everywhere, cosets below q); here are the gate geometries, lookup
widths, cosets and words those never reach.  Every comparison is word for word."""
import contextlib
import itertools
import os
import zlib

import numpy as np
import pytest

import era_boojum_amd as E
import quotient_cases as QC
import quotient_ref as R
from era_boojum_amd import gate_program as GP
from era_boojum_amd.synthetic import GATE_CONSTANT_ALLOCATOR, GATE_FMA, GATE_NOP, GATE_PROGRAM, GATE_REDUCTION4, GateDesc
from gpu_util import DevBuf, ctx

pytestmark = pytest.mark.gpu
P = QC.P
CHALLENGES = pytest.mark.parametrize("noncanonical", [False, True], ids=["canonical_challenges", "challenges_above_p"])
POINTS = (1, 255, 256, 257, 1000)        # one lane, one block short of / exactly / just over a lane, four blocks with a ragged last one


@contextlib.contextmanager
def _switch(name, value):
    """An environment switch of the library for the block (they are read once per process: bj_env_reload re-reads them)."""
    if value is None:
        yield
        return
    os.environ[name] = value
    try:
        E.load_library().bj_env_reload()
        yield
    finally:
        del os.environ[name]
        E.load_library().bj_env_reload()


def _free(bufs):
    for b in bufs:
        b.free()


# ================================================================================================ gates
WIDTH = {GATE_CONSTANT_ALLOCATOR: 1, GATE_FMA: 4, GATE_REDUCTION4: 5}
ROW_CONSTANTS = {GATE_FMA: 2, GATE_REDUCTION4: 4}


def ca(reps, path=(), cs=1):
    return GateDesc(GATE_CONSTANT_ALLOCATOR, "ConstantsAllocatorGate", 1, 1, 1, reps, 1, cs, 1, True, path=list(path))


def fma(reps, path=(), vs=4):
    return GateDesc(GATE_FMA, "FmaGateInBaseFieldWithoutConstant", 3, 2, 4, reps, vs, 0, 1, True, path=list(path))


def red(reps, path=(), cs=0):
    return GateDesc(GATE_REDUCTION4, "ReductionGate<4>", 2, 4, 5, reps, 5, cs, 1, True, path=list(path))


def nop(reps=1, vs=0, path=()):
    return GateDesc(GATE_NOP, "NopGate", 0, 0, 0, reps, vs, 0, 0, True, path=list(path))


def op_list(program, width, reps, n_const=0, path=()):
    return GateDesc(GATE_PROGRAM, "op list", 2, n_const, width, reps, width, 0, program.num_terms, True, path=list(path), program=program)


def _paths(rng, lengths):
    return [[bool(b) for b in rng.integers(0, 2, size=n)] for n in lengths]


def _extent(gates):
    """(variable columns, constant columns) the gates read: the longest path plus the constants behind it"""
    n_vars = n_const = 1
    for g in gates:
        n_const = max(n_const, len(g.path))
        if g.kind == GATE_NOP or g.reps == 0:
            continue
        last = g.reps - 1
        if g.kind == GATE_PROGRAM:
            width, behind = g.principal_width, last * g.const_stride + g.num_constants
        elif g.kind == GATE_CONSTANT_ALLOCATOR:
            width, behind = 1, last * g.const_stride + 1
        else:
            width, behind = WIDTH[g.kind], ROW_CONSTANTS[g.kind]          # row-shared: no per-repetition stride
        n_vars, n_const = max(n_vars, last * g.var_stride + width), max(n_const, len(g.path) + behind)
    return n_vars, n_const


class GateCase:
    def __init__(self, label, gates, points, noncanonical, gap=37, alphas=None, variables=None, constants=None):
        rng = np.random.default_rng([zlib.crc32(label.encode()), points, int(noncanonical)])
        self.label, self.gates, self.points, self.stride = label, gates, points, points + gap
        n_vars, n_const = _extent(gates)
        self.vars = QC.raw_columns(rng, n_vars, self.stride, points, salt=len(label)) if variables is None else variables
        self.consts = QC.raw_columns(rng, n_const, self.stride, points, salt=3) if constants is None else constants
        n_terms = sum(g.reps * g.num_terms for g in gates)
        self.alphas = QC.raw_alphas(rng, n_terms, noncanonical) if alphas is None else alphas
        self.init = QC.raw_columns(rng, 2, self.stride, points, salt=1)        # overwritten: the gate kernels do not accumulate
        self.want = R.to_words(*R.gates_term(self.vars, self.consts, gates, self.alphas, points))


def _run_gate_cases(cases):
    """Every case through the windowed kernel (the default; gate sets it does not take fall back by themselves) and through the
    per-gate kernel (BJ_GATES_WINDOWED=0), each against the reference; the words behind the points stay what they were."""
    C = ctx()
    bufs = [(DevBuf(k.vars), DevBuf(k.consts), DevBuf(k.init)) for k in cases]
    got = {}
    try:
        for windowed in (None, "0"):
            with _switch("BJ_GATES_WINDOWED", windowed):
                for i, (k, (dv, dc, do)) in enumerate(zip(cases, bufs)):
                    C.h2d(do.ptr, k.init)
                    C.quotient_gates(dv.ptr, k.stride, k.vars.shape[0], dc.ptr, k.stride, k.consts.shape[0], k.gates, k.alphas, k.points,
                                     do.ptr, do.ptr + 8 * k.stride)
                    got[i, windowed] = do.get((2, k.stride))
    finally:
        _free(b for t in bufs for b in t)
    for (i, windowed), out in got.items():
        k, kernel = cases[i], "per-gate kernel" if windowed else "default kernel"
        assert np.array_equal(out[:, :k.points], k.want), (k.label, kernel, k.points)
        assert np.array_equal(out[:, k.points:], k.init[:, k.points:]), (k.label, kernel, "words behind the points")


def _gate_of(kind, path):
    """the issue's example: 3 allocations, 6 FMA (24 columns), 5 reductions (25 columns)"""
    return {"c": lambda: ca(3, path), "f": lambda: fma(6, path), "r": lambda: red(5, path)}[kind]()


@CHALLENGES
@pytest.mark.parametrize("points", POINTS)
def test_gate_subsets_and_orders(points, noncanonical):
    """Every non-empty subset of {ConstantsAllocator, FMA, Reduction<4>} and the six orders of all three, with a path length
    and bit pattern of its own per gate (the windowed kernel keeps the path, repetitions and alpha offset per KIND)."""
    rng = np.random.default_rng(points)
    sets = [s for r in (1, 2, 3) for s in itertools.combinations("cfr", r)] + list(itertools.permutations("cfr"))
    cases = []
    for t, kinds in enumerate(sets):
        paths = _paths(rng, [(t + 3 * j) % 7 for j in range(len(kinds))])
        cases.append(GateCase("".join(kinds) + "/%d" % t, [_gate_of(k, p) for k, p in zip(kinds, paths)], points, noncanonical))
    _run_gate_cases(cases)


@CHALLENGES
def test_gate_path_lengths(noncanonical):
    """Selector paths of 0 .. 6 constants for every kind, three different lengths in every gate list."""
    rng = np.random.default_rng(7)
    cases = []
    for L in range(7):
        p = _paths(rng, [L, (L + 2) % 7, (L + 5) % 7])
        cases.append(GateCase("paths %d" % L, [ca(3, p[0]), fma(2, p[1]), red(2, p[2])], 257, noncanonical))
        assert cases[-1].consts.shape[0] == max(L + 3, (L + 2) % 7 + 2, (L + 5) % 7 + 4)   # the longest path plus its constants
    _run_gate_cases(cases)


@CHALLENGES
def test_gate_spans_and_constant_strides(noncanonical):
    """Repetition counts whose column spans end at 1, 19, 20, 21, 40, 41 and 60 — around the windows of 20 columns — and differ
    between the kinds (past the widest span the windowed kernel reads column 0 and must not use it); ConstantsAllocator with one
    shared constant, one per repetition, and every other column."""
    rng = np.random.default_rng(8)
    reps = {1: [(1, None, None)], 19: [(19, 4, 3)], 20: [(7, 5, 2), (3, 2, 4)], 21: [(21, 5, 4)], 40: [(22, 10, 7), (1, 9, 8)],
            41: [(41, 10, 8)], 60: [(60, 15, 12), (2, 3, 12)], 25: [(3, 6, 5)]}
    cases = []
    for span, lists in reps.items():
        for c, f, r in lists:
            p = _paths(rng, [1, 2, 0])
            gates = [ca(c, p[0])] + ([fma(f, p[1])] if f else []) + ([red(r, p[2])] if r else [])
            k = GateCase("span %d: %s" % (span, (c, f, r)), gates, 300, noncanonical)
            assert k.vars.shape[0] == span
            cases.append(k)
    for cs in (0, 1, 2):
        p = _paths(rng, [2, 0, 1])
        k = GateCase("allocator constant stride %d" % cs, [fma(2, p[1]), ca(7, p[0], cs=cs), red(1, p[2])], 300, noncanonical)
        assert k.consts.shape[0] == max(2 + 6 * cs + 1, 5)
        cases.append(k)
    _run_gate_cases(cases)


@CHALLENGES
def test_gate_lists_with_nop_zero_term_and_op_list_gates(noncanonical):
    """Gates that spend no alpha power (NOP, a zero-term gate with repetitions and a path) and gates evaluated by a kernel of
    their own (an op list of one term per repetition, one of two terms and a row constant) between the hand-written ones: those
    behind them must take their own slice of the powers, and the op list's terms are added on top."""
    rng = np.random.default_rng(9)
    p = _paths(rng, [1, 2, 3, 2, 0, 1])
    cases = [
        GateCase("nop and zero-term", [ca(3, p[0]), nop(), fma(6, p[1]), nop(4, 3, p[3]), red(5, p[2])], 257, noncanonical),
        GateCase("op list, one term", [ca(4, p[0]), op_list(GP.selection_program(), 4, 3, path=p[1]), fma(3, p[2]), red(2, p[4])],
                 257, noncanonical),
        GateCase("op list, two terms", [fma(2, p[4]), op_list(GP.uintx_add_program(), 5, 2, n_const=1, path=p[5]), nop(), red(3, p[1]),
                                        ca(5, p[2], cs=2)], 257, noncanonical),
    ]
    assert [sum(g.reps * g.num_terms for g in k.gates) for k in cases] == [14, 12, 14]
    _run_gate_cases(cases)


@CHALLENGES
def test_gate_sets_the_windowed_kernel_does_not_take(noncanonical):
    """Two gates of one kind, a repetition stride other than the gate's width, a Reduction gate with a constant stride: the
    launcher must send them to the per-gate kernel by itself (and the result is the same with the switch set)."""
    rng = np.random.default_rng(10)
    p = _paths(rng, [1, 3, 0, 2, 2, 1])
    _run_gate_cases([
        GateCase("two FMA gates", [fma(3, p[0]), ca(2, p[2]), fma(2, p[1])], 257, noncanonical),
        GateCase("FMA at a stride of 5 columns", [ca(2, p[3]), fma(3, p[4], vs=5)], 257, noncanonical),
        GateCase("Reduction with a constant stride", [red(3, p[5], cs=1), ca(3, p[0])], 257, noncanonical),
    ])


@pytest.mark.parametrize("alpha_word", [P - 1, 2**64 - 1], ids=["alpha_p_minus_1", "alpha_2p64_minus_1"])
def test_gate_accumulators_saturated(alpha_word):
    """60 columns, every term p - 1 and every alpha word as large as it gets: the sums of term * alpha carry into the fifth word
    of the 160-bit accumulators (60 products of almost 2^128 for the allocator, 15 and 12 for the other two)."""
    points, stride = 130, 160
    variables = np.full((60, stride), P - 1, dtype=np.uint64)                  # every variable -1
    constants = np.zeros((7, stride), dtype=np.uint64)
    constants[2], constants[3] = 2, 2
    gates = [ca(60, [], cs=0),                  # v - c[0] = -1
             fma(15, [False]),                  # selector 1 - c[0] = 1;  k0, k1 = c[1], c[2] = 0, 2:  0 * v v + 2 v - v = -1
             red(12, [False, False, True])]     # selector c[2] = 2;  k = c[3..6] = 2, 0, 0, 0:  2 v - v = -1
    for g in gates:
        assert all((t == P - 1).all() for t in R.gate_terms(variables, constants, g, points))
    assert (12 * (P - 1) * alpha_word) >> 128 >= 1
    k = GateCase("saturated", gates, points, False, gap=stride - points, alphas=[(alpha_word, alpha_word)] * 87, variables=variables,
                 constants=constants)
    _run_gate_cases([k])


# ================================================================================================ lookup
def _lookup_columns(rng, w, reps, tid_var, points, stride):
    cps = w + 1 if tid_var else w
    return dict(lvars=QC.raw_columns(rng, reps * cps, stride, points, salt=w), tid=None if tid_var else QC.raw_columns(rng, 1, stride, points, salt=3)[0],
                tables=QC.raw_columns(rng, w + 1, stride, points, salt=reps), mult=QC.raw_columns(rng, 1, stride, points, salt=5)[0])


@CHALLENGES
@pytest.mark.parametrize("w", QC.LOOKUP_WIDTHS)
def test_lookup_term(w, noncanonical):
    """bj_quotient_lookup at widths 1 .. 8 (width 8: lgamma^8, nine table columns), 1, 3 and 11 sub-arguments, the table id as a
    constant column and as the last variable column; A, B and the accumulators are arbitrary words."""
    C = ctx()
    for reps, tid_var, points in itertools.product(QC.LOOKUP_REPS, (False, True), POINTS):
        rng = np.random.default_rng([w, reps, int(tid_var), points, int(noncanonical)])
        stride = points + 29
        k = _lookup_columns(rng, w, reps, tid_var, points, stride)
        AB = QC.raw_columns(rng, 2 * reps + 2, stride, points, salt=7)
        init = QC.raw_columns(rng, 2, stride, points, salt=2)
        lbeta, lgamma = QC.raw_challenge(rng, noncanonical), QC.raw_challenge(rng, noncanonical)
        alphas = QC.raw_alphas(rng, reps + 1, noncanonical)
        want = R.to_words(*R.lookup_term(k["lvars"], k["tid"], k["tables"], k["mult"], AB[:2 * reps], AB[2 * reps:], reps, w, lbeta, lgamma,
                                         alphas, points, (R.res(init[0][:points]), R.res(init[1][:points]))))
        bufs = [DevBuf(k["lvars"]), DevBuf(k["tid"] if not tid_var else np.zeros(1, dtype=np.uint64)), DevBuf(k["tables"]), DevBuf(k["mult"]),
                DevBuf(AB), DevBuf(init)]
        d_l, d_t, d_tab, d_m, d_ab, d_o = bufs
        try:
            C.quotient_lookup(d_l.ptr, stride, None if tid_var else d_t.ptr, d_tab.ptr, stride, d_m.ptr, d_ab.ptr, d_ab.ptr + 8 * stride * 2 * reps,
                              stride, reps, w, lbeta, lgamma, alphas, points, d_o.ptr, d_o.ptr + 8 * stride)
            out = d_o.get((2, stride))
        finally:
            _free(bufs)
        assert np.array_equal(out[:, :points], want), (w, reps, tid_var, points)
        assert np.array_equal(out[:, points:], init[:, points:]), (w, reps, tid_var, points, "words behind the points")


@CHALLENGES
@pytest.mark.parametrize("w", QC.LOOKUP_WIDTHS)
def test_lookup_polynomials(w, noncanonical):
    """bj_lookup_polys over 2^8 rows at the same widths and sub-argument counts (12 denominators: two inversion groups), columns
    at a stride above n; the words behind A and B stay what they were."""
    C = ctx()
    for reps, tid_var in itertools.product(QC.LOOKUP_REPS, (False, True)):
        k = QC.lookup_polys_case(w, reps, tid_var, noncanonical)
        n, stride, tail = k["n"], k["stride"], 16
        wantA, wantB = R.lookup_polys_ref(k["lvars"], k["tid"], k["tables"], k["mult"], reps, w, n, k["lbeta"], k["lgamma"])
        rng = np.random.default_rng(w)
        initA, initB = QC.raw_columns(rng, 1, 2 * reps * n + tail, 0)[0], QC.raw_columns(rng, 1, 2 * n + tail, 0)[0]
        bufs = [DevBuf(k["lvars"]), DevBuf(k["tid"] if not tid_var else np.zeros(1, dtype=np.uint64)), DevBuf(k["tables"]), DevBuf(k["mult"]),
                DevBuf(initA), DevBuf(initB)]
        d_l, d_t, d_tab, d_m, d_A, d_B = bufs
        try:
            C.lookup_polys(d_l.ptr, stride, None if tid_var else d_t.ptr, d_tab.ptr, stride, d_m.ptr, reps, w, QC.LOOKUP_POLYS_LOG_N, k["lbeta"],
                           k["lgamma"], d_A.ptr, d_B.ptr)
            A, B = d_A.get(), d_B.get()
        finally:
            _free(bufs)
        assert np.array_equal(A[:2 * reps * n].reshape(reps, 2, n), wantA) and np.array_equal(B[:2 * n].reshape(2, n), wantB), (w, reps, tid_var)
        assert np.array_equal(A[2 * reps * n:], initA[2 * reps * n:]) and np.array_equal(B[2 * n:], initB[2 * n:]), (w, reps, tid_var)


# ================================================================================================ copy permutation
CP_SHAPES = [(1, 4), (3, 4), (4, 4), (5, 4), (8, 4), (9, 2), (7, 1), (17, 8)]   # (columns, chunk): one chunk (lhs = z(omega x) at once), a
#                                                                                 last chunk of one column, full chunks, chunk = 1
CP_DOMAINS = [(8, 1), (7, 2), (6, 3)]                                            # (log_n, log_lde): 512 points each
SMALL_K = [1, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67]


class CopyPermCase:
    """Columns over the WHOLE LDE domain (global flat index) at a stride above it, and the reference over the whole domain: every
    range of points is then checked against the same slice of it."""

    def __init__(self, V, chunk, log_n, log_lde, noncanonical, non_res=None):
        rng = np.random.default_rng([V, chunk, log_n, log_lde, int(noncanonical)])
        self.V, self.chunk, self.log_n, self.log_lde = V, chunk, log_n, log_lde
        self.n, self.N = 1 << log_n, 1 << (log_n + log_lde)
        self.stride = self.N + 19
        n_chunks = (V + chunk - 1) // chunk
        self.non_res = SMALL_K[:V] if non_res is None else non_res
        self.vars, self.sig = QC.raw_columns(rng, V, self.stride, self.N, salt=V), QC.raw_columns(rng, V, self.stride, self.N, salt=chunk)
        self.s2 = QC.raw_columns(rng, 2 * n_chunks, self.stride, self.N, salt=4)            # z, then n_chunks - 1 partial products
        self.init = QC.raw_columns(rng, 2, self.stride, self.N, salt=6)
        self.beta, self.gamma = QC.raw_challenge(rng, noncanonical), QC.raw_challenge(rng, noncanonical)
        self.alphas = QC.raw_alphas(rng, 1 + n_chunks, noncanonical)
        self.want = R.to_words(*R.copy_perm_term(self.vars, self.sig, self.s2, self.non_res, chunk, log_n, log_lde, self.beta, self.gamma,
                                                 self.alphas, 0, self.N, (R.res(self.init[0][:self.N]), R.res(self.init[1][:self.N]))))
        self.bufs = None

    def upload(self):
        self.bufs = [DevBuf(self.vars), DevBuf(self.sig), DevBuf(self.s2), DevBuf(self.init)]

    def free(self):
        _free(self.bufs or [])

    def run(self, first, count):
        """The points first .. first + count alone, with the pointers at the first of them: they become the reference's words, every
        other word of the accumulators stays what it was."""
        d_v, d_s, d_2, d_o = self.bufs
        C, off = ctx(), 8 * first
        C.h2d(d_o.ptr, self.init)
        C.quotient_copy_perm(d_v.ptr + off, self.stride, d_s.ptr + off, self.stride, d_2.ptr + off, self.stride, self.non_res, self.V,
                             self.chunk, self.log_n, self.log_lde, self.beta, self.gamma, self.alphas, count, first,
                             d_o.ptr + off, d_o.ptr + off + 8 * self.stride)
        expect = self.init.copy()
        expect[:, first:first + count] = self.want[:, first:first + count]
        return d_o.get((2, self.stride)), expect


@CHALLENGES
@pytest.mark.parametrize("V,chunk", CP_SHAPES)
def test_copy_permutation_term_on_every_coset(V, chunk, noncanonical):
    """The whole domain, every coset alone — those at and above q = chunk, which only a rank of a sharded proof evaluates, among
    them — and the first n / 2 points of every coset with the whole coset behind the pointers (8 ranks, q = 4), at LDE factors
    2, 4 and 8."""
    for log_n, log_lde in CP_DOMAINS:
        k = CopyPermCase(V, chunk, log_n, log_lde, noncanonical)
        n, L = k.n, 1 << log_lde
        k.upload()
        try:
            for first, count in [(0, k.N)] + [(c * n, n) for c in range(L)] + [(c * n, n // 2) for c in range(L)]:
                out, expect = k.run(first, count)
                assert np.array_equal(out, expect), (log_n, log_lde, first, count)
        finally:
            k.free()


def _non_residue_sets(V):
    rng = np.random.default_rng(V)
    wide = [int(x) for x in rng.integers(2**32, 2**64, size=V, dtype=np.uint64)]
    wide[0], wide[-1] = 2**64 - 1, P - 1
    return {"small integers": (SMALL_K[:V], True), "2^32 - 1": ([2**32 - 1 - i for i in range(V)], True),
            "2^32": ([2**32 + i for i in range(V)], False), "p + 5": ([P + 5] + [P + 2**32 - 2 - i for i in range(V - 1)], True),
            "64-bit words": (wide, False)}


@CHALLENGES
@pytest.mark.parametrize("name", list(_non_residue_sets(1)))
def test_copy_permutation_term_non_residues(name, noncanonical):
    """Multipliers k_c at the edges of the 32-bit path (it takes every set whose REDUCED words fit 32 bits: p + 5 is 5) and beyond
    it, each set through the default instance and with BJ_COPY_PERM_WIDE_K (the 64 x 64-bit products for any k_c): the same
    words as the reference, hence as each other."""
    for V, chunk in ((5, 4), (17, 8)):
        non_res, fits = _non_residue_sets(V)[name]
        assert all(int(x) % P < 2**32 for x in non_res) == fits
        k = CopyPermCase(V, chunk, 7, 2, noncanonical, non_res=non_res)
        k.upload()
        try:
            for wide in (None, "1"):
                with _switch("BJ_COPY_PERM_WIDE_K", wide):
                    out, expect = k.run(0, k.N)
                    assert np.array_equal(out, expect), (name, V, "wide" if wide else "default")
                    out, expect = k.run(3 * k.n, k.n // 2)
                    assert np.array_equal(out, expect), (name, V, "wide" if wide else "default", "half of coset 3")
        finally:
            k.free()
