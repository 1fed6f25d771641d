"""-m gpu: the five Poseidon2 tree kernels of csrc/poseidon2.hip (poseidon2_leaves_kernel, poseidon2_leaves_chunked_kernel,
poseidon2_nodes_kernel and the lane-parallel poseidon2_nodes_lanepar_kernel, poseidon2_leaves_chunked_lanepar_kernel) at inputs
built to reach their rare paths (tests/poseidon2_tree_cases.py; the CPU side is tests/test_poseidon2_tree_cases.py), and on both
sides of the switch between the per-lane and the lane-parallel kernels.

The lane-parallel kernels have arithmetic of their own (the C++ pow7w with gl::mul_weak's out-of-line branch, lane_matvec +
combine_split for both linear layers, between barriers, four idle lanes per group); the per-lane kernels inline the scheduled
instruction stream, each into its own kernel.  BJ_NODES_LANEPAR_MAX (read through bj_env_reload) picks the kernel of a layer:
`default` puts every shape of this file on the lane-parallel kernels, `0` on the per-lane ones, `64` lets one tree cross the switch
inside its own node layers.

Every comparison is bit-exact on canonical words; every tree is written between guard words that must come back untouched; no
shape exceeds 4096 leaves or parents.  The expected digests of constructed rows come from the integer sponge of the helper, the
whole tree from the oracle.

Not reached: the S-box inputs of rounds >= 1 of the tree kernels (eight free words leave no solve through an S-box layer), and
class 1 at x2*x (no known input)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import era_boojum_amd as E
import oracle as O
from gpu_util import ctx, rand_gl

import poseidon1_layer as PL
import poseidon2_tree_cases as TC
import poseidon_rare as PR
from test_gpu_poseidon_rare_products import WAVE, _spread

pytestmark = pytest.mark.gpu

P = E.P
VAR = "BJ_NODES_LANEPAR_MAX"
BEFORE = os.environ.get(VAR)                                    # what the environment held before this module ran
SETTINGS = {"default": None, "0": "0", "64": "64"}
HASHER_POSEIDON2, HASHER_POSEIDON = 1, 4
GUARD = 16                                                      # words on either side of a tree (digests are stored 16 B wide)
GUARD_WORD, POISON = 0xA5A55A5AC3C33C3C, 0xDEADBEEFDEADBEEF


@contextlib.contextmanager
def lanepar_max(setting, lib=None):
    """BJ_NODES_LANEPAR_MAX as `setting` (`default`: unset) and read by the library for the calls inside, then whatever the
    environment held before, read again.  Must not run beside another call into the library (bj_env_reload)."""
    if lib is None:
        ctx()                                                   # the session's context first: it settles which HIP runtime serves the process
        lib = E.load_library()
    before = os.environ.get(VAR)
    try:
        if SETTINGS[setting] is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = SETTINGS[setting]
        lib.bj_env_reload()
        yield
    finally:
        if before is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = before
        lib.bj_env_reload()


class Guarded:
    """A device buffer of `nwords` between two runs of guard words; `get` asserts the guards and returns the words between."""

    def __init__(self, nwords, init=None):
        host = np.full(nwords + 2 * GUARD, GUARD_WORD, dtype=np.uint64)
        host[GUARD:GUARD + nwords] = POISON if init is None else np.asarray(init, dtype=np.uint64).reshape(-1)
        self.n = nwords
        self.base = ctx().upload(host)
        self.ptr = self.base + 8 * GUARD

    def get(self, shape):
        host = ctx().d2h(self.base, (self.n + 2 * GUARD,))
        ctx().free(self.base)
        assert np.all(host[:GUARD] == GUARD_WORD), "words before the tree were written"
        assert np.all(host[GUARD + self.n:] == GUARD_WORD), "words after the tree were written"
        return host[GUARD:GUARD + self.n].reshape(shape).copy()


def _tree_words(leaves, cap):
    return 4 * ctx().merkle_tree_digests(leaves, cap)


def _build(cols, cap, ptrs=False):
    """merkle_tree_build (or _ptrs) over cols [n_cols, leaves]."""
    c = ctx()
    n_cols, leaves = cols.shape
    d_cols = c.upload(cols)
    out = Guarded(_tree_words(leaves, cap))
    if ptrs:
        c.merkle_tree_build_ptrs([d_cols + 8 * leaves * k for k in range(n_cols)], leaves, cap, out.ptr)
    else:
        c.merkle_tree_build(d_cols, leaves, n_cols, leaves, cap, out.ptr)
    tree = out.get((-1, 4))
    c.free(d_cols)
    return tree


def _chunked(src, log_e, cap):
    """merkle_tree_build_chunked over src [2, len]: leaf j = src[0][jE:(j+1)E] || src[1][jE:(j+1)E]."""
    c = ctx()
    ln = src.shape[1]
    d_src = c.upload(src)
    out = Guarded(_tree_words(ln >> log_e, cap))
    c.merkle_tree_build_chunked(d_src, d_src + 8 * ln, ln, log_e, cap, out.ptr)
    tree = out.get((-1, 4))
    c.free(d_src)
    return tree


def _nodes(kids, cap):
    """merkle_tree_nodes over uploaded digests kids [leaves, 4]."""
    leaves = kids.shape[0]
    host = np.full(_tree_words(leaves, cap), POISON, dtype=np.uint64)
    host[:4 * leaves] = kids.reshape(-1)
    out = Guarded(host.size, host)
    ctx().merkle_tree_nodes(out.ptr, leaves, cap)
    return out.get((-1, 4))


def _rows_as_chunks(rows):
    """Rows of 2E words as the two sources of chunked leaves of E words each."""
    half = rows.shape[1] // 2
    return np.stack([np.ascontiguousarray(rows[:, :half]).reshape(-1), np.ascontiguousarray(rows[:, half:]).reshape(-1)])


def _layout(wave_cases, group_cases, width, rng):
    """Rows of `width` canonical words: `wave_cases` each alone on a lane of a random 64-lane wave and again on a whole wave (four
    workgroups of the lane-parallel kernels), then `group_cases` each alone in a 16-row workgroup-slice and again as all 16 groups
    of a workgroup, padded with random rows to a power of two.  Returns (rows, [(case list, row of the lone case, first row of
    its run, run length)])."""
    fill = lambda n: rand_gl(rng, (n, width))
    a, lone_a, whole_a = _spread([c["words"] for c in wave_cases], fill)
    b, lone_b, whole_b = TC.spread16([c["words"] for c in group_cases], fill)
    rows = np.concatenate([a, b])
    n = 1 << int(rows.shape[0] - 1).bit_length()
    assert a.shape[0] % WAVE == 0 and n <= 4096
    rows = np.concatenate([rows, fill(n - rows.shape[0])])
    return rows, [(wave_cases, lone_a, whole_a, WAVE), (group_cases, lone_b + a.shape[0], whole_b + a.shape[0], TC.GROUPS)]


def _material(wave_cases, group_cases, second_cases, rng):
    """The inputs of one constructed-case test and what they must hash to, computed once per parameter and left unchanged:
    eight-word rows (leaves of eight columns, chunked leaves of 2 x 4 words, child pairs) and sixteen-word rows (chunked leaves
    of 2 x 8 words).  cap 4 for the leaf trees, 8 for the node tree."""
    m = {}
    rows, m["where8"] = _layout(wave_cases, group_cases, 8, rng)
    m["cols"] = np.ascontiguousarray(rows.T)
    m["want_build"] = O.merkle_construct(m["cols"], 4, threads=4)
    m["src4"] = _rows_as_chunks(rows)
    m["want_chunked4"] = O.merkle_construct_chunked(m["src4"], 4, 4, threads=4)
    m["kids"] = rows.reshape(-1, 4)
    m["want_nodes"] = O.merkle_nodes_from_leaf_hashes(m["kids"], 8, threads=4)
    if second_cases is not None:
        rows16, m["where16"] = _layout(second_cases, second_cases, 16, rng)
        m["src8"] = _rows_as_chunks(rows16)
        m["want_chunked8"] = O.merkle_construct_chunked(m["src8"], 8, 4, threads=4)
    for cases in [wave_cases, group_cases] + ([second_cases] if second_cases is not None else []):
        for c in cases:
            c["digest"] = np.array(TC.sponge(TC.rate_blocks(c["words"]))[1], dtype=np.uint64)
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def _check_cases(digests, where, what):
    """digests[r] = the digest of row r: every constructed row carries the integer sponge's digest."""
    for cases, lone, whole, run in where:
        for k, c in enumerate(cases):
            assert np.array_equal(digests[lone[k]], c["digest"]), (what, "lone", run, k)
            assert np.array_equal(digests[whole[k]:whole[k] + run], np.tile(c["digest"], (run, 1))), (what, "whole", run, k)


def _run_material(m, setting):
    """Every entry point over the material under one setting: constructed rows against the integer sponge, trees against the oracle."""
    with lanepar_max(setting):
        got = {"build": _build(m["cols"], 4), "ptrs": _build(m["cols"], 4, ptrs=True), "chunked4": _chunked(m["src4"], 2, 4),
               "nodes": _nodes(m["kids"], 8)}
        if "src8" in m:
            got["chunked8"] = _chunked(m["src8"], 3, 4)
    leaves = m["cols"].shape[1]
    for what in ("build", "ptrs", "chunked4"):
        _check_cases(got[what][:leaves], m["where8"], what)
        assert np.array_equal(got[what], m["want_" + ("build" if what == "ptrs" else what)]), what
    _check_cases(got["nodes"][2 * leaves:3 * leaves], m["where8"], "nodes")
    assert np.array_equal(got["nodes"], m["want_nodes"]), "nodes"
    if "src8" in m:
        _check_cases(got["chunked8"][:m["src8"].shape[1] // 8], m["where16"], "chunked8")
        assert np.array_equal(got["chunked8"], m["want_chunked8"]), "chunked8"


@functools.lru_cache(maxsize=None)
def _sbox_material(cls):
    rng = np.random.default_rng(400 + cls)
    first, second = TC.sbox_cases(cls, rng), TC.sbox_cases(cls, rng, second_block=True)
    assert first and second and all(c["cls"] == cls for c in first + second)
    return _material(first, first, second, rng)


@pytest.mark.parametrize("setting", ["default", "0"])
def test_tree_kernels_at_class_1_sbox_products(setting):
    """Leaves, chunked leaves (first and second block) and child pairs whose first-round S-boxes see an x with x * x in class 1 of
    gl::mul_weak (the final subtraction borrows without the carry: the D - EPS correction applies), on all eight rows of a row
    set or on one word, alone in a wave / 16-lane group and filling whole waves / workgroups."""
    _run_material(_sbox_material(1), setting)


@pytest.mark.parametrize("setting", ["default", "0"])
def test_tree_kernels_at_class_3_sbox_products(setting):
    """The same at class 3 (borrow and carry: the branch is entered, the mask zeroes the correction), at every product of x^7."""
    _run_material(_sbox_material(3), setting)


@functools.lru_cache(maxsize=None)
def _carry_material(lows):
    rng = np.random.default_rng(410 + len(lows))
    cases = {model: TC.carry_cases(model, rng, reps=1, low_halves=(lows,)) for model in TC.CARRY_MODELS}
    return _material(cases["stream_folded"] + cases["stream"], cases["lanepar"], None, rng)


@pytest.mark.parametrize("setting", ["default", "0"])
@pytest.mark.parametrize("lows", ["ones", "random"])
def test_tree_kernels_at_the_carry_of_the_first_external_layer(lows, setting):
    """First blocks whose first external layer wraps in the fold of its plane sums (2^-25 per word on random data) at every output
    word, low halves all ones or random.  The cases of the stream's planes (the constants folded through the matrix, and the
    constant's halves added to the planes) run on lone lanes and whole waves: the per-lane kernels take them, the eight-column
    leaves under both settings, chunked leaves and nodes under `0`.  The cases of lane_matvec + combine_split's planes run on
    lone groups and whole workgroups: the lane-parallel kernels take them under `default`."""
    _run_material(_carry_material(lows), setting)


CHUNKED_SHAPES = [(1, 1), (2, 1), (16, 1), (16, 8), (512, 1), (512, 8)]     # (leaves, cap)


@pytest.mark.parametrize("log_e", range(7))
def test_chunked_leaves_on_both_sides_of_the_switch(log_e):
    """2 x 2^log_e words per leaf (up to sixteen sponge blocks; the zero-padded tail at 2 and 4 words), from one leaf (fifteen dead
    groups that join every barrier and write nothing) to 512: the per-lane kernel, the lane-parallel kernel and a tree that
    crosses the switch in its node layers give the oracle's tree."""
    rng = np.random.default_rng(420 + log_e)
    for leaves, cap in CHUNKED_SHAPES:
        src = rand_gl(rng, (2, leaves << log_e), noncanonical=True)
        want = O.merkle_construct_chunked(src, 1 << log_e, cap, threads=4)
        for setting in SETTINGS:
            with lanepar_max(setting):
                got = _chunked(src, log_e, cap)
            assert np.array_equal(got, want), (leaves, cap, setting)


@pytest.mark.parametrize("leaves", [2, 32, 128, 4096])
def test_node_layers_on_both_sides_of_the_switch(leaves):
    """merkle_tree_nodes over uploaded digests (non-canonical words among them) down to one root and to a cap of leaves / 2."""
    rng = np.random.default_rng(430 + leaves)
    kids = rand_gl(rng, (leaves, 4), noncanonical=True)
    for cap in (1, leaves // 2):
        want = O.merkle_nodes_from_leaf_hashes(kids, cap, threads=4)
        for setting in SETTINGS:
            with lanepar_max(setting):
                got = _nodes(kids, cap)
            assert np.array_equal(got, want), (cap, setting)


class _Recorder:
    """bj_env_reload as a recorder of what the environment held when the library was told to read it."""

    def __init__(self):
        self.seen = []

    def bj_env_reload(self):
        self.seen.append(os.environ.get(VAR))


def test_the_switch_leaves_nothing_behind():
    """The context manager sets, reloads, restores and reloads again, also when its body raises; after every switch test of this
    module the environment holds what it held before the module ran, and the library has read that value; Poseidon (v1), which
    has no lane-parallel kernels, builds the same tree under `0` and `default`."""
    assert os.environ.get(VAR) == BEFORE
    for setting, value in SETTINGS.items():
        rec = _Recorder()
        with lanepar_max(setting, rec):
            assert os.environ.get(VAR) == value
        with pytest.raises(KeyError):
            with lanepar_max(setting, rec):
                raise KeyError(setting)
        assert rec.seen == [value, BEFORE] * 2 and os.environ.get(VAR) == BEFORE
    rng = np.random.default_rng(440)
    cols = rand_gl(rng, (9, 1 << 10), noncanonical=True)
    c = ctx()
    c.set_tree_hasher(HASHER_POSEIDON)
    try:
        trees = []
        for setting in ("0", "default"):
            with lanepar_max(setting):
                trees.append(_build(cols, 16))
    finally:
        c.set_tree_hasher(HASHER_POSEIDON2)
    assert np.array_equal(trees[0], trees[1])
    assert np.array_equal(trees[0], PL.poseidon1_layer().merkle_construct(cols, 16))
    assert os.environ.get(VAR) == BEFORE
    E.load_library().bj_env_reload()                            # the library's view is the environment's, whatever ran before
    assert np.array_equal(_build(cols, 16), O.merkle_construct(cols, 16, threads=4))
