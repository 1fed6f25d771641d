"""Input vectors for operators 12-23 of bj_field_op_batch (tests/test_gpu_field_helpers.py): the csrc/gl.h helpers whose device
compile is not the host's — gl::reduce_limbs / reduce128 and gl::mul_limbs (inline assembly) under gl::Acc160, __brev under
bitrev32 — and the ones no test calls directly (mul_u32_weak, mul7_weak, mul_pow2, mul7, pow7, the inversion chains).

Everything is plain Python integers.  The module also carries MODELS of the device algorithms, word for word, which label every
vector with the branch it takes; tests/test_field_helper_cases.py proves on the CPU that the vectors reach every branch and that
a model with a branch's correction taken out fails on exactly that branch's vectors, so a pass on the GPU is no accident of the
inputs.  Random operands reach the rare branches of the reduction about once in 2^32."""
import json
import os
import random

from test_gpu_field_ops import SPECIALS

P = (1 << 64) - (1 << 32) + 1
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
EPS = M32                      # 2^64 mod p
HERE = os.path.dirname(os.path.abspath(__file__))


def rare_pairs():
    """(a, b) of tests/golden/gl_mul_rare.json: products whose reduction borrows."""
    with open(os.path.join(HERE, "golden", "gl_mul_rare.json")) as f:
        return [(v["a"], v["b"]) for v in json.load(f)["vectors"]]


# ---- gl::reduce_limbs(hi_hi, hi_lo, lo), device branch --------------------------------------------------------------------
CLASSES = ["plain", "carry", "ge", "borrow+plain", "borrow+carry", "borrow+ge"]


def reduce_model(hi_hi, hi_lo, lo, ge_fix=True, borrow_fix=True):
    """The device algorithm: t = lo - hi_hi (+ p on a borrow);  r, carry = t + hi_lo * (2^32 - 1) in one multiply-add;  + EPS
    when the sum carried or when r >= p.  Returns (result, class).  ge_fix / borrow_fix = False leave that correction out."""
    borrow = lo < hi_hi
    t = (lo - hi_hi) & M64
    if borrow and borrow_fix:
        t = (t - EPS) & M64            # borrowed 2^64 = p + EPS: cannot borrow again, t was >= 2^64 - 2^32 + 1
    full = t + hi_lo * EPS
    carry, r = full >> 64, full & M64
    ge = r >= P
    assert not (carry and ge)          # a carried sum is below 2^64 - 2^33
    fix = EPS if (carry or (ge and ge_fix)) else 0
    return (r + fix) & M64, ("borrow+" if borrow else "") + ("carry" if carry else "ge" if ge else "plain")


LIMBS = [0, 1, 2, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]
# the intermediate r made p - 1, p, p + 1, 2^64 - 1, and wrapped to 0 and to 1
R_TARGETS = [P - 1, P, P + 1, M64, M64 + 1, M64 + 2]


def reduction_grid():
    """(hi_hi, hi_lo, lo): the limb edges x the edge words, and for every limb pair the lo that puts r on each target — once
    for a difference that does not borrow and once (EPS more) for one that does."""
    out, seen = [], set()
    for hh in LIMBS:
        for hl in LIMBS:
            los = list(SPECIALS)
            for target in R_TARGETS:
                los.append((target - hl * EPS + hh) & M64)
                los.append((target - hl * EPS + hh + EPS) & M64)
            for lo in los:
                if (hh, hl, lo) not in seen:
                    seen.add((hh, hl, lo))
                    out.append((hh, hl, lo))
    return out


def reduce_value(v):
    hh, hl, lo = v
    return (hh << 96) + (hl << 64) + lo


def by_class(vectors, cls_of):
    out = {c: [] for c in CLASSES}
    for v in vectors:
        out[cls_of(v)].append(v)
    return out


def interleave(classes, waves=6):
    """waves x 64 vectors, lane j of every wave from class (j + wave) % 6: every mask of the reduction differs from lane to lane."""
    out = []
    for w in range(waves):
        for lane in range(64):
            c = classes[CLASSES[(lane + w) % len(CLASSES)]]
            out.append(c[(w * 64 + lane) % len(c)])
    return out


# ---- gl::Acc160: (w4, w3, w2, w1:w0, x, y) --------------------------------------------------------------------------------
W4S = [0, 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]


def acc_state(v):
    w4, w3, w2, w10 = v[:4]
    return (w4 << 128) + (w3 << 96) + (w2 << 64) + w10


def acc_sum(v):
    return acc_state(v) + v[4] * v[5]


def acc160_model(v):
    """fma(x, y) on the five words, then reduce(): reduce_limbs of the low four, minus w4 * 2^32 (2^128 = -2^32 mod p).
    Returns (result, class of the reduction)."""
    s = acc_sum(v)
    assert s < (1 << 160)
    r, cls = reduce_model((s >> 96) & M32, (s >> 64) & M32, s & M64)
    return (r - ((s >> 128) << 32)) % P, cls        # gl::sub on canonical operands: (w4 << 32) <= p - 1


def closed_form_all_ones(k):
    """The state after k products of 2^64 - 1 by itself, as (w4, w3, w2, w1:w0)."""
    s = k * M64 * M64
    assert s < (1 << 160)
    return (s >> 128, (s >> 96) & M32, (s >> 64) & M32, s & M64)


def accumulator_grid():
    """Returns (kept, dropped): the combinations below 2^160, which the accumulator's contract covers, and the ones it excludes."""
    grid = reduction_grid()
    rare = rare_pairs()
    rng = random.Random(160)
    out = []
    for w4 in W4S:
        for i, (hh, hl, lo) in enumerate(grid):
            out.append((w4, hh, hl, lo, 0, 0))                     # reduce() alone: the reduction grid under every top word
            out.append((w4, hh, hl, lo, M64, M64))
            out.append((w4, hh, hl, lo) + rare[(i + w4) % len(rare)])
    ones = [(1, 1), (1, M64), (M64, M64), (1 << 32, 1 << 32), (1 << 63, 2), (0, 0)] + rare
    for w4 in W4S:                                                 # one product carries through four words into w4
        for x, y in ones:
            out.append((w4, M32, M32, M64, x, y))
            out.append((w4, M32, M32, M64 - 1, x, y))
    for k in (1, 2, (1 << 31), (1 << 32) - 2, (1 << 32) - 1):      # k all-ones products in closed form, then one more
        out.append(closed_form_all_ones(k) + (M64, M64))
        out.append(closed_form_all_ones(k) + (0, 0))
    for _ in range(1 << 15):
        kind = rng.randrange(4)
        w4 = rng.getrandbits(32) if kind else rng.choice(W4S)
        x, y = (rng.getrandbits(64), rng.getrandbits(64)) if kind != 1 else rng.choice(rare)
        out.append((w4, rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(64), x, y))
    kept = [v for v in out if acc_sum(v) < (1 << 160)]
    return kept, [v for v in out if acc_sum(v) >= (1 << 160)]


def acc_ext2_cases():
    """(t0, t1, a0, a1): every slot an edge word most of the time, any u64 otherwise; a1 is canonicalised by the kernel."""
    rng = random.Random(14)
    edge = SPECIALS + [M64 - 1, (1 << 64) - (1 << 32) - 1]
    out = [(a, a, a, a) for a in edge]
    out += [(M64, M64, M64, P - 1), (M64, M64, M64, M64), (P - 1, P - 1, P - 1, P - 1), (0, M64, 0, P - 1), (M64, 0, P - 1, 0)]
    while len(out) < 8192:
        out.append(tuple(rng.choice(edge) if rng.random() < 0.6 else rng.getrandbits(64) for _ in range(4)))
    return out


def acc_ext2_want(v):
    t0, t1, a0, a1 = v
    a1 %= P
    return 2 * (t0 * a0 + 7 * t1 * a1) % P, 2 * (t0 * a1 + t1 * a0) % P


# ---- gl::mul_u32_weak / mul7_weak ------------------------------------------------------------------------------------------
def mul_u32_weak_model(a, k):
    """Two 32 x 32 products, the bits above 2^64 folded back with 2^64 = EPS.  Returns (weak residue, whether s + t wrapped)."""
    lo = (a & M32) * k
    hi = (a >> 32) * k + (lo >> 32)
    t = (hi >> 32) * EPS
    s = ((lo & M32) | ((hi & M32) << 32)) + t
    wrapped = s > M64
    s &= M64
    if wrapped:
        assert s + EPS <= M64          # no second wrap
        s += EPS
    return s, wrapped


def _wrapping_operands(k):
    """a with k * a = c * 2^64 + 0xFFFFFFFF'xxxxxxxx: the packed low words sit within 2^32 of 2^64 and the fold wraps them."""
    out = []
    for c in (range(1, k) if k <= 16 else sorted({1, 2, k // 2, k - 2, k - 1})):
        for low in (0, 1, 1 << 16, 1 << 31, M32 - k):                # the low word of the product, about
            a = -(-((c << 64) + (M32 << 32) + low) // k)
            if a <= M64:
                out.append(a)
    return out


KS = [0, 1, 7, 11, 13, 1 << 31, (1 << 32) - 2, (1 << 32) - 1]


def mul_u32_cases():
    rng = random.Random(16)
    ks = KS + [rng.getrandbits(32) for _ in range(24)]
    words = SPECIALS + [rng.getrandbits(64) for _ in range(40)]
    out = [(a, k) for k in ks for a in words + _wrapping_operands(k)]
    out += [(rng.getrandbits(64), rng.getrandbits(32)) for _ in range(1 << 14)]
    out += [(a, k + (rng.getrandbits(32) << 32)) for a, k in out[:64]]      # the kernel takes the low 32 bits of b
    return out


def mul7_lazy_cases():
    rng = random.Random(15)
    return SPECIALS + _wrapping_operands(7) + [rng.getrandbits(64) for _ in range(1 << 14)]


# ---- the rest -----------------------------------------------------------------------------------------------------------
def mul_pow2_cases():
    """(a, k): every shift on the edge words (canonicalised by the kernel) and on random canonical words."""
    rng = random.Random(17)
    words = SPECIALS + [rng.randrange(P) for _ in range(200)]
    return [(a, k) for k in range(32) for a in words] + [(a, k + 32 * j) for j, (a, k) in enumerate((w, 5) for w in SPECIALS)]


def mul7_cases():
    rng = random.Random(18)
    return [0, 1, P - 1, P // 7 - 1, P // 7, P // 7 + 1] + SPECIALS + [rng.randrange(P) for _ in range(4096)]


def pow7_cases():
    rng = random.Random(19)
    return mul7_cases() + [P + rng.getrandbits(31) for _ in range(256)] + [rng.getrandbits(64) for _ in range(1024)]


INV_SPECIALS = [0, 1, 2, 7, P - 1, P - 2, 0xFFFFFFFF, 0x100000000]


def inverse_cases():
    rng = random.Random(20)
    return INV_SPECIALS + [P, P + 1, M64] + [rng.randrange(P) for _ in range(2048)]


def ext2_inverse_cases():
    rng = random.Random(21)
    out = [(a, b) for a in INV_SPECIALS for b in INV_SPECIALS]
    out += [(P, P), (P + 1, M64), (M64, 0), (0, M64)]                # canonicalised by the kernel
    return out + [(rng.randrange(P), rng.randrange(P)) for _ in range(2048)]


def ext2_inverse_want(v):
    c0, c1 = v[0] % P, v[1] % P
    ni = pow((c0 * c0 - 7 * c1 * c1) % P, P - 2, P)                  # the norm is 0 only for (0, 0): 7 is no square
    return c0 * ni % P, -c1 * ni % P


def bitrev_cases():
    """(x, bits): all widths 0..32; the kernel takes the low 32 bits of x."""
    rng = random.Random(23)
    xs = [0, 1, M32, 1 << 31, 0x80000001, 0x12345678] + [rng.getrandbits(32) for _ in range(10)]
    xs += [x | (rng.getrandbits(32) << 32) for x in xs[:6]]
    return [(x, bits) for bits in range(33) for x in xs]


def bitrev_want(v):
    x, bits = v
    return sum(((x >> i) & 1) << (bits - 1 - i) for i in range(bits))
