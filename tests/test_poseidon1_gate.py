"""PoseidonFlattenedGate<F, 8, 12, 4, PoseidonGoldilocks> (src/cs/gates/poseidon.rs:12-500), the Poseidon (v1) round-function gate:
the fused partial-round constants (tools/gen_poseidon1_fused_constants.py) against the plain permutation, the traced evaluator
(gate_program.evaluate_poseidon_flattened) against a second restatement written here, the synthetic witness fill, and the
routing of its capture to the hand-written evaluator (csrc/gate_poseidon.hip) by fingerprint."""
import ctypes as C
import random

import numpy as np

import oracle
from era_boojum_amd import gate_program as G, synthetic as S

import reference_capture as RC

P = G.P
rnd = random.Random(20261016)


def fused_permutation(state):
    """poseidon_permutation_optimized (poseidon_goldilocks.rs:374-420) with the generated tables."""
    rc = G.poseidon2_round_constants()
    fused_rc, dense, sbox_rc, vs, w_hats = G.poseidon1_fused_constants()
    m = G.poseidon1_mds_matrix()
    mds = lambda s: [sum(m[r][k] * s[k] for k in range(12)) % P for r in range(12)]
    s = [x % P for x in state]
    for r in range(3):
        s = mds([pow(x + rc[r][i], 7, P) for i, x in enumerate(s)])
    s = [(pow(x + rc[3][i], 7, P) + fused_rc[i]) % P for i, x in enumerate(s)]
    s = [sum(dense[r][k] * s[k] for k in range(12)) % P for r in range(12)]
    for r in range(22):
        s0 = (pow(s[0], 7, P) + sbox_rc[r]) % P
        s = [(s0 + sum(vs[r][k - 1] * s[k] for k in range(1, 12))) % P] + [(s[k] + w_hats[r][k - 1] * s0) % P for k in range(1, 12)]
    s = mds([pow(x, 7, P) for x in s])
    for r in range(27, 30):
        s = mds([pow(x + rc[r][i], 7, P) for i, x in enumerate(s)])
    return s


def test_fused_constants_give_the_permutation():
    """test_valid_transformation (poseidon_goldilocks.rs:1035-1050), on 1 000 random states and a few edge ones."""
    states = [[rnd.randrange(P) for _ in range(12)] for _ in range(1000)] + [[0] * 12, [1] * 12, [P - 1] * 12]
    for st in states:
        want = [int(x) for x in oracle.poseidon_permutation(np.array(st, dtype=np.uint64))]
        assert fused_permutation(st) == want


def test_generated_table_is_current():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_poseidon1_fused_constants.py")
    spec = importlib.util.spec_from_file_location("gen_p1", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rc, dense, sbox_rc, vs, w_hats = gen.fused_constants()
    assert G.poseidon1_fused_constants() == (rc, dense, sbox_rc, vs, w_hats)


def restated_terms(v, wit=(), num_witness_columns_used=0):
    """poseidon.rs:199-464 a second time, in python integers: the 118 terms of one repetition."""
    rc = G.poseidon2_round_constants()
    fused_rc, dense, sbox_rc, vs, w_hats = G.poseidon1_fused_constants()
    exps = [0, 0, 1, 0, 3, 5, 1, 8, 12, 3, 16, 10]
    mds = lambda s: [sum(s[k] << exps[(k - r) % 12] for k in range(12)) % P for r in range(12)]
    cells = list(wit[:num_witness_columns_used]) + list(v[24:])
    terms, state = [], [x % P for x in v[:12]]

    def reset(idx):
        for i in idx:
            cell = cells.pop(0) % P
            terms.append((state[i] - cell) % P)
            state[i] = cell
    for r in range(4):
        if r:
            reset(range(12))
        state[:] = [pow(x + rc[r][i], 7, P) for i, x in enumerate(state)]
        if r < 3:
            state[:] = mds(state)
    t = [(x + fused_rc[i]) % P for i, x in enumerate(state)]
    state[:] = [sum(dense[r][k] * t[k] for k in range(12)) % P for r in range(12)]
    for r in range(22):
        reset([0])
        s0 = (pow(state[0], 7, P) + sbox_rc[r]) % P
        state[:] = [(s0 + sum(vs[r][k - 1] * state[k] for k in range(1, 12))) % P] + \
                   [(state[k] + w_hats[r][k - 1] * s0) % P for k in range(1, 12)]
    for k in range(4):
        reset(range(12))
        state[:] = mds([pow(x + (rc[26 + k][i] if k else 0), 7, P) for i, x in enumerate(state)])
    terms += [(v[12 + i] - state[i]) % P for i in range(12)]
    assert not cells and len(terms) == 118
    return terms


def _satisfying_rows(m, w=0, seed=0):
    rng = np.random.default_rng(seed)
    fill = S._CellFill([rng.integers(0, P, size=m, dtype=np.uint64) for _ in range(12)], m)
    G.evaluate_poseidon_flattened(fill, w)
    var = [fill.cells[("var", k)] for k in range(130 - w)]
    wit = [fill.cells[("wit", k)] for k in range(w)]
    return var, wit


def test_traced_program_shape_and_terms():
    prog, compact = G.poseidon_flattened_program(), G.poseidon_flattened_compact_program()
    assert prog.num_terms == compact.num_terms == 118
    refs = [r for _, _, a, b in prog.relations for r in (a, b)] + list(prog.writes)
    assert max(i for k, i in refs if k == G.IDX_VARIABLE) + 1 == 130 and prog.witness_width == 0
    for _ in range(4):                                       # arbitrary (unsatisfying) rows
        v = [rnd.randrange(P) for _ in range(130)]
        want = restated_terms(v)
        assert prog.evaluate(v, []) == want and compact.evaluate(v, []) == want
    var, _ = _satisfying_rows(16)
    for j in range(16):                                      # satisfying rows: the output cells are the permutation
        v = [int(c[j]) for c in var]
        assert prog.evaluate(v, []) == [0] * 118 and compact.evaluate(v, []) == [0] * 118
        assert v[12:24] == [int(x) for x in oracle.poseidon_permutation(np.array(v[:12], dtype=np.uint64))]


def test_witness_column_variant():
    w = 20
    prog = G.poseidon_flattened_program(w)
    assert prog.witness_width == w and prog.num_terms == 118
    for _ in range(3):
        v, wit = [rnd.randrange(P) for _ in range(130 - w)], [rnd.randrange(P) for _ in range(w)]
        assert prog.evaluate(v, [], wit) == restated_terms(v[:24] + v[24:], wit, w)
    var, wit = _satisfying_rows(8, w)
    for j in range(8):
        assert prog.evaluate([int(c[j]) for c in var], [], [int(c[j]) for c in wit]) == [0] * 118


def test_recursion_class_circuits_with_the_v1_gate_are_satisfied():
    for variant in ("kind", "op_list", 12):
        c = S.recursion_like_circuit(8, seed=5, poseidon1=variant)
        g = c.gates[2]
        assert g.name.startswith("PoseidonFlattenedGate") and g.program is not None
        assert g.kind == (S.GATE_POSEIDON_FLATTENED if variant == "kind" else S.GATE_PROGRAM)
        S.check_satisfied(c)
    m = np.ones(c.n, dtype=bool)
    for i, bit in enumerate(g.path):
        m &= c.constants[i] == (1 if bit else 0)
    c.variables[60, int(np.flatnonzero(m)[1])] ^= np.uint64(1)
    try:
        S.check_satisfied(c)
        raise AssertionError("a broken v1 row must be caught")
    except AssertionError as e:
        assert "unsatisfied" in str(e)


def test_fingerprint_routes_the_capture_to_the_hand_written_evaluator():
    import era_boojum_amd as E
    from era_boojum_amd import gate_codegen as GC
    lib = E.load_library()
    prog = G.poseidon_flattened_program()
    assert lib.bj_gate_program_generated(C.byref(prog.struct)) == 1                       # -> csrc/gate_poseidon.hip
    assert lib.bj_gate_program_generated(C.byref(G.poseidon_flattened_program(12).struct)) == 0     # witness cells: op list
    assert lib.bj_gate_program_generated(C.byref(G.poseidon_flattened_compact_program().struct)) == 0
    fp = GC.program_fingerprint(prog)
    assert fp != GC.program_fingerprint(G.poseidon2_flattened_program())
    src = open(GC.OUT).read()
    assert "bool gate_is_poseidon_flattened(uint64_t fp0, uint64_t fp1) { return fp0 == 0x%016xULL && fp1 == 0x%016xULL; }" % fp in src
    # the reference's numbering (a process-wide temporary counter, sparse or dense): the same function, the same fingerprint
    cap = RC.capture(G.evaluate_poseidon_flattened, 0)
    for p in (RC.to_program(cap), RC.to_program_raw(cap)):
        assert GC.program_fingerprint(p) == fp
        assert lib.bj_gate_program_generated(C.byref(p.struct)) == 1
    v = [rnd.randrange(P) for _ in range(130)]
    assert RC.to_program(cap).evaluate(v, []) == restated_terms(v)


def test_the_library_reports_the_new_gate_kind():
    """Gate kinds are added within an ABI version: a host asks bj_gate_kind_supported for the one it needs."""
    import era_boojum_amd as E
    lib = E.load_library()
    assert [lib.bj_gate_kind_supported(k) for k in range(9)] == [0, 1, 1, 1, 1, 1, 1, 1, 0]
    assert lib.bj_gate_kind_supported(S.GATE_POSEIDON_FLATTENED) == 1
