"""Inputs that drive the rare paths of the five Poseidon2 tree kernels of csrc/poseidon2.hip (leaves, chunked leaves, nodes and
the two lane-parallel kernels), in python integers on top of tests/poseidon_rare.py.  CPU only; the host test is
tests/test_poseidon2_tree_cases.py, the GPU side tests/test_gpu_poseidon2_tree_kernels.py.

  * `sponge`: the Poseidon2 sponge from its definition (initial external layer, 4 + 22 + 4 rounds, internal matrix
    1 + diag(2^SH), overwrite absorption at rate 8, zero-padded tail, no length tag).  It returns the twelve first-round S-box
    inputs EXT * state + RC[0] of every block and the digest: the expected value of every constructed case, independent of the
    C oracle.
  * S-box cases: a node or a first leaf block has capacity 0, so eight words are free and eight of the twelve first-round S-box
    inputs can be prescribed.  414 of the 495 eight-row submatrices of EXT[:, 0:8] are singular mod p; rows 0-7 and rows 4-11
    are invertible and cover all twelve words together (`ROW_SETS`, asserted at import).  A case puts a target x on all eight
    rows of a set, or on one row with the other seven targets random.  For the second block of a 16-word leaf the capacity
    after the first permutation comes from the model and the system stays affine in the block's eight words.  Targets are
    >= 2^32 - 1: such a residue has one 64-bit representative, so the device's S-box input word is x whatever the lazy
    arithmetic did before and poseidon_rare.mul_weak_model applies to the products of x^7.
  * Carry cases: first blocks (words 8-11 zero) whose first external layer wraps in the fold of its low / high plane sums at a
    chosen output word, under a model of the planes: `stream_carry_words` (the round constant's halves added to the planes, the
    model tests/test_gpu_poseidon2.py builds its permutation states with), `lanepar_carry_words` for lane_matvec + combine_split of
    the lane-parallel kernels (no constant), and `stream_folded_carry_words`, which restates the planes of the generated stream
    of the per-lane kernels exactly: the stream folds the constants through the matrix, so its plane sums differ from the first
    model's although the residue is the same.
  * `spread16`: the layout for kernels that run one item per 16 lanes, sixteen items per workgroup.

Not reachable by construction: the S-box inputs of rounds >= 1.  With eight free words (capacity 0, or fixed by the block before)
there is no linear solve through an S-box layer, so those rounds see the constructed rows as random data; class 1 at x2*x has no
known input at all (tests/test_poseidon_rare_products.py)."""
import json
import os

import numpy as np

import poseidon_rare as PR
from poseidon_rare import EXT, P, RC

EPS = 0xFFFFFFFF
MIN_TARGET = (1 << 32) - 1
SH = [4, 14, 11, 8, 0, 5, 2, 9, 13, 6, 3, 12]                  # poseidon2/params.rs:38-39
ROW_SETS = (tuple(range(0, 8)), tuple(range(4, 12)))
LONE_WORDS = (0, 5, 8, 11)
RARE_MUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gl_mul_rare.json")


# ---- the sponge from its definition
def _ext(s):
    return [sum(m * v for m, v in zip(row, s)) % P for row in EXT]


def permutation(state):
    """(output residues, first-round S-box inputs EXT * state + RC[0]) of the Poseidon2 permutation on any integers."""
    s = _ext([x % P for x in state])
    first = None
    for r in range(30):
        if r < 4 or r >= 26:
            s = [(x + RC[r][k]) % P for k, x in enumerate(s)]
            first = first or list(s)
            s = _ext([pow(x, 7, P) for x in s])
        else:
            s[0] = pow((s[0] + RC[r][0]) % P, 7, P)
            tot = sum(s)
            s = [(tot + (x << SH[k])) % P for k, x in enumerate(s)]
    return s, first


def rate_blocks(words):
    """A leaf's words as rate blocks of eight, the last one zero-padded."""
    words = [int(w) for w in words]
    return [words[t:t + 8] + [0] * (8 - len(words[t:t + 8])) for t in range(0, len(words), 8)]


def sponge(blocks):
    """(first-round S-box inputs of every block's permutation, digest) of the overwrite sponge over `blocks` of eight words."""
    s, log = [0] * 12, []
    for b in blocks:
        assert len(b) == 8
        s, first = permutation(list(b) + s[8:])
        log.append(first)
    return log, s[:4]


def capacity_after(blocks):
    s = [0] * 12
    for b in blocks:
        s = permutation(list(b) + s[8:])[0]
    return s[8:]


# ---- S-box cases
def _sub(rows):
    return [[EXT[i][j] for j in range(8)] for i in rows]


for _rows in ROW_SETS:                                          # both systems are invertible: solve_mod_p finds every pivot
    PR.solve_mod_p(_sub(_rows), [0] * 8)
assert set(ROW_SETS[0]) | set(ROW_SETS[1]) == set(range(12))


def solve_block(rows, targets, capacity=(0, 0, 0, 0)):
    """The eight rate words whose permutation, on top of `capacity`, sees targets[k] at the first-round S-box of word rows[k]."""
    rhs = [(t - RC[0][i] - sum(EXT[i][8 + k] * capacity[k] for k in range(4))) % P for i, t in zip(rows, targets)]
    return PR.solve_mod_p(_sub(rows), rhs)


def sbox_targets(cls):
    """[(x, product whose operands take class `cls`)]: the weak-chain entries of the S-box fixture, the operands of
    gl_mul_rare.json whose own square takes the class (the S-box's first product is x * x), and for class 1 also 2^48 and
    3 * 2^48; only x >= 2^32 - 1."""
    out = [(e["x"], e["product"]) for e in PR.entries("weak", cls)]
    with open(RARE_MUL) as f:
        vectors = [v for v in json.load(f)["vectors"] if v["class"] == cls]
    extra = [v["a"] % P for v in vectors] + ([1 << 48, 3 << 48] if cls == 1 else [])
    for x in extra:
        if PR.mul_weak_model(x, x)[1] == cls:
            out.append((x, "x*x"))
    seen, uniq = set(), []
    for x, prod in out:
        if x >= MIN_TARGET and x not in seen:
            seen.add(x)
            uniq.append((x, prod))
    return uniq


def _rand_words(rng, n):
    return [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]


def sbox_cases(cls, rng, second_block=False):
    """Constructed leaves / child pairs: dicts with `words` (8, or 16 with `second_block`), `block` (the sponge block whose
    permutation sees the target), `rows` (the S-box words that see it), `x`, `product`, `cls`."""
    cases = []
    for x, prod in sbox_targets(cls):
        shapes = [(rows, rows) for rows in ROW_SETS]
        shapes += [(ROW_SETS[0] if w < 8 else ROW_SETS[1], (w,)) for w in LONE_WORDS]
        for rows, hit in shapes:
            first = _rand_words(rng, 8) if second_block else []
            cap = capacity_after([first]) if second_block else (0, 0, 0, 0)
            targets = [x if i in hit else int(rng.integers(MIN_TARGET, P, dtype=np.uint64)) for i in rows]
            cases.append({"words": first + solve_block(rows, targets, cap), "block": int(second_block), "rows": tuple(hit),
                          "x": x, "product": prod, "cls": cls})
    return cases


# ---- carry cases of the first external layer
def plane_sums(state, k_lo, k_hi):
    """(A_i, B_i) of the first external layer: the sums of the low and of the high 32-bit halves of the state under row i of EXT,
    each plus that plane's constant of the kernel (k_lo[i], k_hi[i]).  A_i + 2^32 * B_i is the layer's output before the fold."""
    return [(sum(EXT[i][j] * (state[j] & EPS) for j in range(12)) + k_lo[i],
             sum(EXT[i][j] * (state[j] >> 32) for j in range(12)) + k_hi[i]) for i in range(12)]


def _wrapping_words(state, k_lo, k_hi):
    """The fold T = A + B.hi * EPS, then one add T.hi + B.lo on the high word: the words where that add wraps."""
    return [i for i, (A, B) in enumerate(plane_sums(state, k_lo, k_hi)) if ((A + (B >> 32) * EPS) >> 32) + (B & EPS) >= 1 << 32]


def stream_constants(rc):
    return [r & EPS for r in rc], [r >> 32 for r in rc]


def stream_carry_words(state, rc):
    """Which output words of the first external layer wrap in the fold of their low / high plane sums (tools/gen_p2_asm.py
    `combine`: T = A + B.hi * EPS, then T.hi + B.lo >= 2^32) — a model of the planes, not of the field arithmetic."""
    return _wrapping_words(state, *stream_constants(rc))


def folded_constants(rc):
    """The plane constants of the generated stream, which folds the round constants THROUGH the matrix (tools/gen_p2_asm.py
    fold_ext_constants and ext_layer): with C = EXT^-1 rc and D_b = C_b + sum_b' C_b', block b computes M4 (x_b + sum_b' x_b' + D_b)
    on each plane, D_0 entering as its two halves and D_b - D_0 (mod p) as its two halves for b = 1, 2."""
    C = PR.solve_mod_p(EXT, rc)
    tot = [(C[j] + C[4 + j] + C[8 + j]) % P for j in range(4)]
    D = [[(C[4 * b + j] + tot[j]) % P for j in range(4)] for b in range(3)]
    k_lo, k_hi = [], []
    for b in range(3):
        diff = [(D[b][j] - D[0][j]) % P if b else 0 for j in range(4)]
        for i in range(4):
            k_lo.append(sum(PR.M4[i][j] * ((D[0][j] & EPS) + (diff[j] & EPS)) for j in range(4)))
            k_hi.append(sum(PR.M4[i][j] * ((D[0][j] >> 32) + (diff[j] >> 32)) for j in range(4)))
    return k_lo, k_hi


def stream_folded_carry_words(state, rc):
    """The same fold over the planes as the generated stream forms them (`folded_constants`): the model that decides whether the
    per-lane kernels take the out-of-line carry.  `stream_carry_words` adds the constant's own halves instead, which is the
    same residue from other plane sums."""
    return _wrapping_words(state, *folded_constants(rc))


def lanepar_carry_words(state, rc=None):
    """The same for lane_matvec + combine_split (csrc/poseidon2.hip): the planes carry no constant, which addw_rc adds to the
    folded word afterwards."""
    return _wrapping_words(state, [0] * 12, [0] * 12)


CARRY_MODELS = {"stream": stream_carry_words, "stream_folded": stream_folded_carry_words, "lanepar": lanepar_carry_words}
CARRY_CONSTANTS = {"stream": stream_constants, "stream_folded": folded_constants, "lanepar": lambda rc: ([0] * 12, [0] * 12)}


def carry_cases(model, rng, reps=4, low_halves=("ones", "random")):
    """For every output word i, `reps` first blocks (eight canonical words, words 8-11 zero) that wrap at word i under `model`:
    low halves all 0xFFFFFFFF or random in [2^31, 2^32) (rep r takes low_halves[r mod len]), high halves random but the one under
    an odd entry of row i among columns 0-7, solved mod 2^32 so that lo32(B_i) = 2^32 - 1 - small.  Asserts that every case wraps
    at its word and that the cases reach all twelve words.  Dicts with `words`, `word`, `model`."""
    wraps = CARRY_MODELS[model]
    k_hi = CARRY_CONSTANTS[model](RC[0])[1]
    cases = []
    for rep in range(reps):
        for i in range(12):
            while True:
                hi = [int(rng.integers(0, 1 << 32)) for _ in range(8)]
                lo = [EPS if low_halves[rep % len(low_halves)] == "ones" else int(rng.integers(1 << 31, 1 << 32)) for _ in range(8)]
                js = next(j for j in range(8) if EXT[i][j] % 2 == 1)          # an odd entry is invertible mod 2^32
                rest = sum(EXT[i][j] * hi[j] for j in range(8) if j != js) + k_hi[i]
                want_lo = (EPS - int(rng.integers(0, 8))) & EPS
                hi[js] = (want_lo - rest) * pow(EXT[i][js], -1, 1 << 32) % (1 << 32)
                words = [(h << 32) | l for h, l in zip(hi, lo)]
                if all(w < P for w in words):
                    break
            assert i in wraps(words + [0] * 4, RC[0]), (model, i)
            cases.append({"words": words, "word": i, "model": model})
    reached = set()
    for c in cases:
        reached.update(wraps(c["words"] + [0] * 4, RC[0]))
    assert reached == set(range(12)), (model, reached)
    return cases


# ---- layout for the kernels that run one item per 16 lanes
GROUPS = 16                                                     # BJ_LANEPAR_GROUPS: items per 256-lane workgroup


def spread16(cases, fill):
    """Rows (row r = node or leaf r): workgroup-slice c (16 rows) holds case c on one row among random rows (`fill(n)`), slice
    len(cases) + c holds case c on all 16 rows.  Returns (rows, row of the lone case c, first row of its whole slice)."""
    cases = np.asarray(cases, dtype=np.uint64)
    n = len(cases)
    rows = fill(2 * n * GROUPS)
    lone = np.array([GROUPS * c + (7 * c + 3) % GROUPS for c in range(n)])
    whole = np.array([GROUPS * (n + c) for c in range(n)])
    rows[lone] = cases
    for c in range(n):
        rows[whole[c]:whole[c] + GROUPS] = cases[c]
    return rows, lone, whole
