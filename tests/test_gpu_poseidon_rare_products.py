"""-m gpu: the rare branches of gl::mul_weak (csrc/gl.h) inside the Poseidon kernels, at inputs built to reach them
(tests/poseidon_rare.py, fixture tests/golden/poseidon_sbox_rare.json; the CPU side is tests/test_poseidon_rare_products.py).
Class 1 = the final subtraction borrows without the carry (the D - EPS correction applies), class 3 = borrow and carry (the
branch is entered, the mask zeroes the correction).  Each test takes one class, so a wrong correction or a wrong mask fails the
tests of its own class.  Expected values come from integers or the oracle; comparisons are bit-exact.  Every constructed case
runs on a lone lane of an otherwise random wave and on a whole wave of its own, in launches over many workgroups.

A wrong class-1 correction changes the residue, so the class-1 tests catch it in every context.  In class 3 the masked
correction only picks the representative: D + EPS mod 2^64 (the correct sequence) and D - EPS + EPS = D (the sequence without
its s_andn2_b64) are congruent, as D >= p.  By value, the class-3 tests therefore check that the entered branch leaves every
other register, mask and loop of the kernel intact, as with the missing SCC clobber of the past.  That the mask is zeroed is
asserted on the emulated sequence (tests/test_poseidon_rare_products.py).

Not reached here: class 1 at x2*x (no known construction, ~2^-64 at random); rounds >= 2 of leaf and node hashing (capacity
words fixed at 0 leave no solve through two S-box layers: the same inlined permutation is driven at every round through
poseidon_permute).  Poseidon2's tree kernels (BJ_HASHER_POSEIDON2: leaves, chunked leaves and nodes, per lane and lane-parallel,
each with the permutation inlined or restated on its own) are driven at constructed first-round inputs in
tests/test_gpu_poseidon2_tree_kernels.py; the tree test below is BJ_HASHER_POSEIDON (v1) only.  The group-wise absorb kernels (poseidon1_ and poseidon2_leaves_absorb_kernel) are reached in
tests/test_gpu_prover_only_kernels.py: bj_merkle_leaves_absorb with first = 0, last = 1 takes the capacity words from the
caller, so the constructed twelve-word states of the permutation tests go through both kernels at every round, on lone lanes
and whole waves."""
import ctypes as C
import functools

import numpy as np
import pytest

import era_boojum_amd as E
import oracle as O
from era_boojum_amd import gate_program as GP, synthetic as S
from gpu_util import DevBuf, ctx, rand_gl
from oracle import gates as OG

import poseidon1_layer as PL
import poseidon_rare as PR
from test_poseidon1_gate import restated_terms

pytestmark = pytest.mark.gpu

P = E.P
WAVE = 64
HASHER_POSEIDON = 4


def _spread(cases, fill):
    """Rows: wave c holds case c on one lane among random rows (`fill(n)`), wave len(cases) + c holds case c on every lane.
    Returns (rows, lane index of case c, first index of its whole wave)."""
    cases = np.asarray(cases, dtype=np.uint64)
    n = len(cases)
    rows = fill(2 * n * WAVE)
    lone = np.array([WAVE * c + (7 * c + 3) % WAVE for c in range(n)])
    whole = np.array([WAVE * (n + c) for c in range(n)])
    rows[lone] = cases
    for c in range(n):
        rows[whole[c]:whole[c] + WAVE] = cases[c]
    return rows, lone, whole


def _check_cases(got, lone, whole, want):
    """want[c]: the expected row of case c, on its lone lane and on all of its whole wave."""
    for c in range(len(want)):
        assert np.array_equal(got[lone[c]], want[c]), ("lone lane", c)
        assert np.array_equal(got[whole[c]:whole[c] + WAVE], np.tile(want[c], (WAVE, 1))), ("whole wave", c)


V1_ROUNDS = [0, 1, 3, 4, 15, 25, 26, 29]     # first loop, partial loop first / middle / last, last loop


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cls", [1, 3])
def test_v1_permutation_at_rare_sbox_products(cls):
    """Context.poseidon_permute (poseidon1_permute_states_kernel): a fixture value at the S-box input of one word (word 0 in the
    partial rounds) and of all twelve words of the target round, other words random, against oracle.poseidon_permutation
    and poseidon1_layer.poseidon1_many_np."""
    rng = np.random.default_rng(100 + cls)
    cases = []
    for ent in PR.entries("weak", cls):
        for r in V1_ROUNDS:
            for words in (([r % 12], range(12)) if PR.is_full(r) else ([0],)):
                st = PR.v1_construct(r, list(words), ent["x"], rng)
                assert all(PR.v1_forward(st)[1][r][k] == ent["x"] for k in words)
                cases.append(st)
    rows, lone, whole = _spread(cases, lambda n: rand_gl(rng, (n, 12), noncanonical=True))
    rows = np.concatenate([rows, rand_gl(rng, (max(0, 32 * 256 - rows.shape[0]), 12), noncanonical=True)])   # 32 workgroups
    d = DevBuf(rows)
    ctx().poseidon_permute(d.ptr, rows.shape[0])
    got = d.get(rows.shape)
    d.free()
    _check_cases(got, lone, whole, [O.poseidon_permutation(np.array(s, dtype=np.uint64)) for s in cases])
    assert np.array_equal(got, PL.poseidon1_many_np(rows))


@pytest.mark.timeout(120)
def test_v1_permutation_on_extreme_words():
    """As Poseidon2's test_permutation_on_extreme_words: boundary words in most positions, so that a missed double carry or
    borrow of the weak arithmetic would show."""
    specials = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 2, P - 1, P, P + 1, (1 << 64) - (1 << 32), (1 << 64) - 2,
                (1 << 64) - 1, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF, 0xFFFFFFFEFFFFFFFF, 1 << 48]
    rng = np.random.default_rng(78)
    st = np.zeros((4096, 12), dtype=np.uint64)
    for i in range(st.shape[0]):
        for k in range(12):
            st[i, k] = specials[int(rng.integers(0, len(specials)))] if rng.random() < 0.8 else int(rng.integers(0, 1 << 63)) * 2 + 1
    st[0], st[1], st[2] = (1 << 64) - 1, P - 1, P
    d = DevBuf(st)
    ctx().poseidon_permute(d.ptr, st.shape[0])
    got = d.get(st.shape)
    d.free()
    assert np.array_equal(got, np.stack([O.poseidon_permutation(s) for s in st]))


def _leaf_cases(cls, width, rng):
    """Leaf rows of `width` words whose first permutation sees a fixture value at round 0 (all rate words) or round 1 (one
    word); with width >= 9 also the second absorption's round 0 (its rate words after the first eight)."""
    cases = []
    for x in sorted({e["x"] for e in PR.entries("weak", cls)}):
        free = min(width, 8)
        cases.append([PR.tree_round0_word(k, x) for k in range(free)] + [int(v) for v in rng.integers(0, P, size=width - free, dtype=np.uint64)])
        for j in (0, 5, 11):
            cases.append(PR.tree_round1_words(j, x, rng, free) + [int(v) for v in rng.integers(0, P, size=width - free, dtype=np.uint64)])
        if width > 8:
            first = [int(v) for v in rng.integers(0, P, size=8, dtype=np.uint64)]
            cases.append(first + [PR.tree_round0_word(k, x) for k in range(width - 8)])
    return cases


def _pad_pow2(rows, rng, least=4096):
    """Random rows up to a power of two of at least `least` leaves (16 workgroups)."""
    n = max(least, 1 << int(rows.shape[0] - 1).bit_length())
    return np.concatenate([rows, rand_gl(rng, (n - rows.shape[0], rows.shape[1]))]) if n > rows.shape[0] else rows


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cls", [1, 3])
def test_v1_tree_entry_points_at_rare_sbox_products(cls):
    """BJ_HASHER_POSEIDON: merkle_tree_build and merkle_tree_build_ptrs with 8 and 12 columns (the second absorption's round 0),
    merkle_tree_build_chunked (8 and 16 words per leaf) and merkle_tree_nodes over uploaded child digests, against
    tests/poseidon1_layer.py."""
    layer = PL.poseidon1_layer()
    c = ctx()
    rng = np.random.default_rng(200 + cls)
    cap = 4
    c.set_tree_hasher(HASHER_POSEIDON)
    bufs = []
    try:
        for width in (8, 12):
            rows, _, _ = _spread(_leaf_cases(cls, width, rng), lambda n: rand_gl(rng, (n, width)))
            rows = _pad_pow2(rows, rng)
            leaves = rows.shape[0]
            cols = np.ascontiguousarray(rows.T)
            want = layer.merkle_construct(cols, cap)
            nd = c.merkle_tree_digests(leaves, cap)
            d_tree = c.malloc(32 * nd)
            bufs.append(d_tree)
            d_cols = c.upload(cols)
            bufs.append(d_cols)
            c.merkle_tree_build(d_cols, leaves, width, leaves, cap, d_tree)
            assert np.array_equal(c.d2h(d_tree, (nd, 4)), want), ("strided", width)
            d_tree2 = c.upload(np.zeros((nd, 4), dtype=np.uint64))
            bufs.append(d_tree2)
            c.merkle_tree_build_ptrs([d_cols + 8 * leaves * k for k in range(width)], leaves, cap, d_tree2)
            assert np.array_equal(c.d2h(d_tree2, (nd, 4)), want), ("ptrs", width)
            if width == 8:                                      # the same rows as chunked leaves of 2 x 4 words
                src = [np.ascontiguousarray(rows[:, :4]).reshape(-1), np.ascontiguousarray(rows[:, 4:]).reshape(-1)]
                d_src = c.upload(np.stack(src))
                bufs.append(d_src)
                c.merkle_tree_build_chunked(d_src, d_src + 8 * src[0].size, src[0].size, 2, cap, d_tree)
                assert np.array_equal(c.d2h(d_tree, (nd, 4)), layer.merkle_construct_chunked(np.stack(src), 4, cap)), "chunked 4"
        # 16 words per leaf: two absorptions, the second one's round 0 driven
        rows, _, _ = _spread([r + [int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)] for r in _leaf_cases(cls, 12, rng)],
                             lambda n: rand_gl(rng, (n, 16)))
        rows = _pad_pow2(rows, rng)
        leaves = rows.shape[0]
        src = np.stack([np.ascontiguousarray(rows[:, :8]).reshape(-1), np.ascontiguousarray(rows[:, 8:]).reshape(-1)])
        d_src = c.upload(src)
        bufs.append(d_src)
        nd = c.merkle_tree_digests(leaves, cap)
        d_tree = c.malloc(32 * nd)
        bufs.append(d_tree)
        c.merkle_tree_build_chunked(d_src, d_src + 8 * src.shape[1], src.shape[1], 3, cap, d_tree)
        assert np.array_equal(c.d2h(d_tree, (nd, 4)), layer.merkle_construct_chunked(src, 8, cap)), "chunked 8"
        # nodes: the first level's parents see the target at round 0 or 1 (children = 8 state words)
        parents, lone, whole = _spread(_leaf_cases(cls, 8, rng), lambda n: rand_gl(rng, (n, 8)))
        parents = _pad_pow2(parents, rng)
        kids = parents.reshape(-1, 4)
        leaves = kids.shape[0]
        nd = c.merkle_tree_digests(leaves, cap)
        tree = np.zeros((nd, 4), dtype=np.uint64)
        tree[:leaves] = kids
        d_tree = c.upload(tree)
        bufs.append(d_tree)
        c.merkle_tree_nodes(d_tree, leaves, cap)
        got = c.d2h(d_tree, (nd, 4))
        assert np.array_equal(got, layer._nodes(kids, cap)), "nodes"
        assert np.array_equal(got[leaves:leaves + parents.shape[0]], PL.poseidon1_many_c(np.concatenate(
            [parents, np.zeros((parents.shape[0], 4), dtype=np.uint64)], axis=1))[:, :4])
    finally:
        c.set_tree_hasher(1)
        for b in bufs:
            c.free(b)


# ---- the flattened gates through bj_quotient_gates, the interpreter and the run-time compiled programs
GATE_FORMS = [("v1", "kind"), ("v1", "capture"), ("v1", "compact"), ("v1", "interpreter"),
              ("p2", "capture"), ("p2", "compact"), ("p2", "interpreter")]
PATH = [True, True]                                             # selector = c0 * c1


def _rare_pairs(cls):
    """Constant pairs (c0, c1) whose selector product c0 * c1 takes class `cls`: 2^48 * 2^48 = -1 for class 1, the class-3
    pairs of tests/golden/gl_mul_rare.json."""
    if cls == 1:
        pairs = [(1 << 48, 1 << 48), (3 << 48, 1 << 48)]
    else:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gl_mul_rare.json")) as f:
            pairs = [(v["a"], v["b"]) for v in json.load(f)["vectors"] if v["class"] == 3 and v["a"] < P and v["b"] < P]
    assert pairs and all(PR.mul_weak_model(a, b)[1] == cls for a, b in pairs)
    return pairs


def _alphas(rng):
    a = rand_gl(rng, (118, 2))
    for j in range(118):
        a[j, 0] = [0, 1, P - 1, a[j, 0]][j % 4]
        a[j, 1] = [a[j, 1], P - 1, 0, 1][j % 4]
    return a


def _terms(gate, v):
    return restated_terms(v) if gate == "v1" else [t[0] for t in OG.ev_poseidon2_flattened([(x % P, 0) for x in v], [])]


@functools.lru_cache(maxsize=None)
def _gate_points(gate, cls):
    """Constructed points: a fixture value of the canonical chain at one S-box input of every slot (full rounds 0-3 and 26-29,
    partial iterations first / middle / last), and at every S-box input at once; a rare selector product on every third
    point; variables below 2^32 - 1 given as their non-canonical representative v + p (the fixture's 2^14 and 2^24 in the
    partial slots among them), and the output cells so as well.  Returns (var (130, n), con (2, n), alphas, constructed
    indices, expected (2, n) at those indices as python ints, terms at those indices)."""
    rng = np.random.default_rng(300 + cls + (0 if gate == "v1" else 10))
    pts = []
    for ent in PR.entries("canonical", cls):
        for slot in PR.SLOTS:
            i = 0 if slot[0] == "partial" else (slot[1] + ent["position"]) % 12
            pts.append(PR.gate_point(gate, [(slot, i, ent["x"])], rng))
        pts.append(PR.gate_point(gate, [(s, i, ent["x"]) for s in PR.SLOTS for i in range(1 if s[0] == "partial" else 12)], rng))
    pairs = _rare_pairs(cls)
    cons = [pairs[k // 3 % len(pairs)] if k % 3 == 0 else tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64))
            for k in range(len(pts))]
    shown = []
    for v in pts:
        for k in range(12, 24, 3):                              # output cells: small residues, non-canonical words
            small = int(rng.integers(0, (1 << 32) - 1))
            v[k] = small
        shown.append([x + P if x < (1 << 32) - 1 else x for x in v])
    cases = np.array([w + list(cc) for w, cc in zip(shown, cons)], dtype=np.uint64)
    rows, lone, whole = _spread(cases, lambda n: np.concatenate([rand_gl(rng, (n, 130), noncanonical=True),
                                                                 rand_gl(rng, (n, 2), noncanonical=True)], axis=1))
    var, con = np.ascontiguousarray(rows[:, :130].T), np.ascontiguousarray(rows[:, 130:].T)
    alphas = _alphas(rng)
    terms, want = [], []
    for v, (c0, c1) in zip(pts, cons):
        t = _terms(gate, v)
        sel = (c0 % P) * (c1 % P) % P
        terms.append(t)
        want.append([sel * sum(int(alphas[j, k]) * t[j] for j in range(118)) % P for k in range(2)])
    return var, con, alphas, lone, whole, want, terms


def _program(gate, form):
    if form == "compact":
        return GP.poseidon_flattened_compact_program() if gate == "v1" else GP.poseidon2_flattened_compact_program()
    return GP.poseidon_flattened_program() if gate == "v1" else GP.poseidon2_flattened_program()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("cls", [1, 3])
@pytest.mark.parametrize("gate,form", GATE_FORMS)
def test_flattened_gate_at_rare_sbox_products(gate, form, cls):
    """sel * sum alpha_t * term_t at every constructed point (lone lane and whole wave) from the hand-written kernels (v1 as
    kind 7 and as its capture, Poseidon2 as its capture, routed by fingerprint), the run-time compiled compact programs and
    the interpreter's raw terms (combined here), against restated_terms / oracle.gates.ev_poseidon2_flattened in integers."""
    var, con, alphas, lone, whole, want, terms = _gate_points(gate, cls)
    n = var.shape[1]
    assert n >= 20 * 256
    lib = E.load_library()
    d_var, d_con = DevBuf(var), DevBuf(con)
    try:
        if form == "interpreter":
            d_terms = DevBuf(nelems=118 * n)
            ctx().gate_program_eval(_program(gate, form), d_var.ptr, n, d_con.ptr, n, 1, 130, 0, n, d_terms.ptr)
            raw = d_terms.get((118, n))
            d_terms.free()
            for c in range(len(want)):
                for i in [lone[c]] + list(range(whole[c], whole[c] + WAVE)):
                    t = [int(x) for x in raw[:, i]]
                    assert t == terms[c], (c, i)
                    sel = (int(con[0, i]) % P) * (int(con[1, i]) % P) % P
                    got = [sel * sum(int(alphas[j, k]) * t[j] for j in range(118)) % P for k in range(2)]
                    assert got == want[c], (c, i)
            return
        if form == "kind":
            g = S.GateDesc(S.GATE_POSEIDON_FLATTENED, "PoseidonFlattenedGate", 7, 0, 130, 1, 130, 0, 118, True, path=PATH)
        else:
            prog = _program(gate, form)
            assert lib.bj_gate_program_generated(C.byref(prog.struct)) == (1 if form == "capture" else 0)
            g = S.GateDesc(S.GATE_PROGRAM, "PoseidonFlattenedGate" if gate == "v1" else "Poseidon2FlattenedGate", 7, 0, 130, 1, 130,
                           0, 118, True, path=PATH, program=prog)
        d_out = DevBuf(nelems=2 * n)
        ctx().quotient_gates(d_var.ptr, n, 130, d_con.ptr, n, 2, [g], alphas, n, d_out.ptr, d_out.ptr + 8 * n)
        got = d_out.get((2, n)).T
        d_out.free()
        _check_cases(got, lone, whole, np.array(want, dtype=np.uint64))
    finally:
        d_var.free()
        d_con.free()


@pytest.mark.timeout(300)
def test_hand_written_poseidon2_quotient_equals_the_interpreter_on_random_points():
    """As test_gpu_poseidon1_gate.py's v1 test, for gate_poseidon.hip: unsatisfying random LDE inputs (not reduced); the
    kernel's selector * sum alpha_t * term_t equals the same sum over the interpreter's raw terms at every point, and those
    terms equal the golden-pinned oracle evaluator at every point."""
    n, path = 1500, [True, False]
    rng = np.random.default_rng(79)
    var = rand_gl(rng, (130, n), noncanonical=True)
    con = rand_gl(rng, (2, n), noncanonical=True)
    alphas = rand_gl(rng, (118, 2))
    d_var, d_con, d_out = DevBuf(var), DevBuf(con), DevBuf(nelems=2 * n)
    prog = GP.poseidon2_flattened_program()
    assert E.load_library().bj_gate_program_generated(C.byref(prog.struct)) == 1
    gate = S.GateDesc(S.GATE_PROGRAM, "Poseidon2FlattenedGate", 7, 0, 130, 1, 130, 0, 118, True, path=path, program=prog)
    ctx().quotient_gates(d_var.ptr, n, 130, d_con.ptr, n, 2, [gate], alphas, n, d_out.ptr, d_out.ptr + 8 * n)
    got = d_out.get((2, n))
    d_terms = DevBuf(nelems=118 * n)
    ctx().gate_program_eval(prog, d_var.ptr, n, d_con.ptr, n, 1, 130, 0, n, d_terms.ptr)
    terms = d_terms.get((118, n))
    for i in range(n):
        t = [int(x) for x in terms[:, i]]
        assert t == _terms("p2", [int(x) for x in var[:, i]]), i
        sel = (int(con[0, i]) % P) * ((1 - int(con[1, i])) % P) % P
        for k in range(2):
            assert int(got[k, i]) == sel * sum(int(alphas[j, k]) * t[j] for j in range(118)) % P, (i, k)
    for b in (d_var, d_con, d_out, d_terms):
        b.free()
