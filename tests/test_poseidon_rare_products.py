"""The rare branches of gl::mul_weak (csrc/gl.h) inside the Poseidon S-boxes, on the CPU: every entry of the fixture of
tools/find_poseidon_sbox_rare.c (tests/golden/poseidon_sbox_rare.json) run through the real instruction sequence of gl.h on the
single-lane emulator (tools/p2_emulate.py), and the constructions of tests/poseidon_rare.py that place its values at chosen
S-box inputs, checked against integers and the oracle.  The GPU side is tests/test_gpu_poseidon_rare_products.py.

Cells: chain (weak = poseidon1.hip p1_pow7, canonical = the gates' pow7) x product (x*x, x2*x, x2*x2, x4*x3) x class (1 = borrow
without carry, the D - EPS correction applies; 3 = borrow with carry, the branch is entered and the mask zeroes it).  Every
class-3 cell has entries; class 1 has x*x in both chains and x2*x2, x4*x3 in the canonical chain (2^24, 2^14: the weak chain
only sees words >= 2^32 - 1 there).  The one allowed gap: class 1 at x2*x, which has no known construction (~2^-64 at random)."""
import os
import sys

import numpy as np
import pytest

import oracle as O
from era_boojum_amd import gate_program as G
from oracle import gates as OG

import poseidon_rare as PR
from test_poseidon1_gate import restated_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import p2_emulate as EM   # noqa: E402

P = PR.P
GAP = ("x2*x", 1)


def _emulated_mul_weak():
    src = open(os.path.join(ROOT, "era_boojum_amd", "csrc", "gl.h")).read()
    lines = EM.asm_lines_of(src, "__device__ __forceinline__ u64 mul_weak(u64 a, u64 b)")
    e, regs = EM.bind_sequence(lines, ["a0", "a1", "b0", "b1"], ["out"], ["cm", "c"])
    out = int(regs["out"][2:regs["out"].index(":")])
    log = []

    def mul(a, b):
        for n, val in (("a", a), ("b", b)):
            e.v[int(regs[n + "0"][1:])], e.v[int(regs[n + "1"][1:])] = val & 0xFFFFFFFF, val >> 32
        e.execute()
        entered = e.counts["VALU"] == 17                       # 14 in line + the 3 of the out-of-line correction
        assert e.counts["VALU"] in (14, 17)
        log.append((entered, entered and e.v[53] == 0xFFFFFFFF))  # v53: the correction mask the branch builds
        return e.v[out] | (e.v[out + 1] << 32)
    return mul, log


def test_fixture_covers_every_cell_but_the_one_gap():
    have = {(e["chain"], e["product"], e["class"]) for e in PR.fixture()}
    for chain in ("weak", "canonical"):
        for prod in PR.PRODUCTS:
            assert (chain, prod, 3) in have, (chain, prod)
    assert {(c, p) for c, p, k in have if k == 1} == {("weak", "x*x"), ("canonical", "x*x"), ("canonical", "x2*x2"),
                                                      ("canonical", "x4*x3")}
    assert all((e["product"], e["class"]) != GAP for e in PR.fixture())
    for e in PR.fixture():
        assert 0 <= e["x"] < P and PR.PRODUCTS[e["position"]] == e["product"]
        if e["chain"] == "weak":
            assert e["x"] >= (1 << 32) - 1                     # its only u64 representative: the device sees exactly x


@pytest.mark.parametrize("chain", ["weak", "canonical"])
def test_fixture_enters_the_branch_of_the_gl_h_sequence(chain):
    """Each entry's x^7 on the emulated gl.h sequence: the stated product executes the 3 out-of-line instructions, its
    correction mask is raised exactly in class 1, and every product of the chain is congruent to the integer product."""
    mul, log = _emulated_mul_weak()
    for ent in PR.entries(chain, 1) + PR.entries(chain, 3):
        log.clear()
        ops = PR.pow7_operands(ent["x"], chain, mul)
        assert ops == PR.pow7_operands(ent["x"], chain)       # the model of the C tool is the sequence
        for (a, b), (entered, corrected) in zip(ops, log):
            assert PR.mul_weak_model(a, b)[1] & 1 == entered
            assert corrected == (entered and PR.mul_weak_model(a, b)[1] == 1)
        log.clear()
        for a, b in ops:
            assert mul(a, b) % P == a * b % P
        entered, corrected = log[ent["position"]]
        assert entered, ent
        assert corrected == (ent["class"] == 1), ent
        assert PR.mul_weak_model(*ops[ent["position"]])[1] == ent["class"]
        x = ent["x"]
        x2 = x * x % P
        assert [a * b % P for a, b in ops] == [x2, x2 * x % P, x2 * x2 % P, pow(x, 7, P)]


# target rounds of the v1 permutation: first full-round loop, partial loop (first / middle / last), last loop
V1_ROUNDS = [0, 1, 3, 4, 15, 25, 26, 29]


def test_v1_backward_construction_reaches_the_target_rounds():
    rng = np.random.default_rng(11)
    for ent in PR.entries("weak", 1) + PR.entries("weak", 3):
        for r in V1_ROUNDS:
            for words in ([r % 12] if PR.is_full(r) else [0], range(12) if PR.is_full(r) else [0]):
                st = PR.v1_construct(r, list(words), ent["x"], rng)
                out, log = PR.v1_forward(st)
                assert all(log[r][k] == ent["x"] for k in words), (r, ent)
                assert out == [int(v) for v in O.poseidon_permutation(np.array(st, dtype=np.uint64))]


def test_tree_constructions_reach_rounds_0_and_1_with_zero_capacity():
    rng = np.random.default_rng(12)
    for ent in PR.entries("weak", 1) + PR.entries("weak", 3):
        x = ent["x"]
        for j in range(12):
            st = PR.tree_round1_words(j, x, rng) + [0] * 4
            out, log = PR.v1_forward(st)
            assert log[1][j] == x and out == [int(v) for v in O.poseidon_permutation(np.array(st, dtype=np.uint64))]
        for free in (1, 5):                                   # a short second absorption: zero padding beyond `free`
            st = PR.tree_round1_words(free - 1, x, rng, free) + [0] * (12 - free)
            assert PR.v1_forward(st)[1][1][free - 1] == x
        st = [PR.tree_round0_word(k, x) for k in range(8)] + [0] * 4
        assert PR.v1_forward(st)[1][0][:8] == [x] * 8


@pytest.mark.parametrize("gate", ["v1", "p2"])
def test_gate_constructions_reach_every_round_class(gate):
    """Every slot (full rounds 0-3 and 26-29, partial iterations first / middle / last) of both gates: the S-box inputs
    restated from the variables hit the target, and the two pinned term evaluators agree with the traced programs there."""
    rng = np.random.default_rng(13)
    prog = G.poseidon_flattened_program() if gate == "v1" else G.poseidon2_flattened_program()
    for ent in PR.entries("canonical", 1) + PR.entries("canonical", 3):
        for slot in PR.SLOTS:
            i = 0 if slot[0] == "partial" else (slot[1] + ent["position"]) % 12
            v = PR.gate_point(gate, [(slot, i, ent["x"])], rng)
            assert PR.gate_sbox_inputs(gate, v, slot)[i] == ent["x"], (slot, ent)
    v = PR.gate_point(gate, [(s, i, 1 << 48) for s in PR.SLOTS for i in range(1 if s[0] == "partial" else 12)], rng)
    for s in PR.SLOTS:
        assert set(PR.gate_sbox_inputs(gate, v, s)) == {1 << 48}
    want = restated_terms(v) if gate == "v1" else [t[0] for t in OG.ev_poseidon2_flattened([(x, 0) for x in v], [])]
    assert prog.evaluate(v, []) == want
