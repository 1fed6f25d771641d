"""Shared by tests/test_verify_host.py and tests/test_gpu_verify.py: keys and proof words for bj_verify."""
import types

import numpy as np

from era_boojum_amd import proof_format, synthetic as S

P = (1 << 64) - (1 << 32) + 1
GOLDEN_GENERAL_GATES = ["ConstantsAllocatorGate", "U8x4FMAGate", "Poseidon2FlattenedGate", "DotProductGate<4>", "ZeroCheckGate",
                        "FmaGateInBaseFieldWithoutConstant", "UIntXAddGate", "SelectionGate", "ParallelSelectionGate<4>", "NopGate",
                        "ReductionGate<4>"]   # evaluator order of the golden proof's inner circuit (tests/test_oracle_fixture.py)


def golden_proof_dict(fx):
    return {"proof_config": fx["proof_config"], "public_inputs": fx["public_inputs"],
            "witness_oracle_cap": fx["witness_oracle_cap"], "stage_2_oracle_cap": fx["stage_2_oracle_cap"],
            "quotient_oracle_cap": fx["quotient_oracle_cap"], "values_at_z": fx["values_at_z"],
            "values_at_z_omega": fx["values_at_z_omega"], "values_at_0": fx["values_at_0"],
            "fri_base_oracle_cap": fx["fri_base_oracle_cap"], "fri_intermediate_oracles_caps": fx["fri_intermediate_oracles_caps"],
            "final_fri_monomials": fx["final_fri_monomials"], "pow_challenge": fx["pow_challenge"],
            "queries_per_fri_repetition": fx["queries"]}


def golden_circuit(fx, with_boolean_gate=True):
    """The bj_circuit side of the golden inner circuit (what oracle.verifier.vk_from_reference_geometry reads out of the fixture):
    geometry and selector paths from `selectors_placement` (left = the constant), the evaluators of GOLDEN_GENERAL_GATES in that
    order with the descriptors of synthetic.recursion_gates by name, the Boolean gate over one specialized column, non_residues(155, n).
    with_boolean_gate=False: the same column under an evaluator whose one term is a - a — the key of a circuit that lacks the
    Boolean constraint (an op list without relations is refused, and the column has to belong to some gate)."""
    from era_boojum_amd import gate_program as GP
    g = fx["geometry"]
    n = g["domain_size"]
    lk = g["lookup"]["UseSpecializedColumnsWithTableIdAsConstant"]
    paths = {}

    def walk(node, prefix):
        if "GateOnly" in node:
            paths[node["GateOnly"]["gate_idx"]] = list(prefix)
        elif "Fork" in node:
            walk(node["Fork"]["left"], prefix + [True])
            walk(node["Fork"]["right"], prefix + [False])
    walk(g["selectors_placement"], [])
    by_name = {d.name: d for d in S.recursion_gates(g["num_variable_columns"], g["num_constant_columns"])}
    gates = []
    for idx, name in enumerate(GOLDEN_GENERAL_GATES):
        d = by_name[name]
        d.path = paths.get(idx, [])
        gates.append(d)
    if with_boolean_gate:
        boolean = S.GateDesc(S.GATE_PROGRAM, "BooleanConstraintGate", 2, 0, 1, 1, 1, 0, 1, False, program=GP.boolean_program())
    else:
        boolean = S.GateDesc(S.GATE_PROGRAM, "NoConstraint", 1, 0, 1, 1, 1, 0, 1, False,
                             program=GP.GateProgram([(GP.OP_SUB, 0, (0, 0), (0, 0))], [], [(3, 0)], 1))
    vgp = g["num_variable_columns"]
    num_vars = vgp + lk["width"] * lk["num_repetitions"] + 1
    return types.SimpleNamespace(
        log_n=n.bit_length() - 1, n=n, num_vars=num_vars, num_gp_vars=vgp, num_witness_cols=0,
        num_constant_cols=g["num_constant_columns"] + g["extra_constant_polys_for_selectors"] + len(g["table_ids_column_idxes"]),
        lookup_width=lk["width"], lookup_reps=lk["num_repetitions"], table_id_col=g["table_ids_column_idxes"][0],
        quotient_degree=g["quotient_degree"], gates=gates, non_residues=S.non_residues(num_vars, n),
        public_inputs=[(c, r, 0) for c, r in g["public_inputs_locations"]], specialized_gates=[boolean])


def golden_config(fx):
    cfg = fx["proof_config"]
    return dict(fri_lde_factor=cfg["fri_lde_factor"], cap_size=cfg["merkle_tree_cap_size"], security_level=cfg["security_level"],
                pow_bits=cfg["pow_bits"], transcript="poseidon2")


def bump(words, pos):
    """words with position pos set to (canonical value + 1) mod p."""
    out = np.array(words, dtype=np.uint64, copy=True)
    out[pos] = np.uint64((int(out[pos]) % P + 1) % P)
    return out


class Layout:
    """Word ranges of a BJPF v2 buffer by field class (era_boojum_amd/proof_format.py), for tests that edit proofs."""

    def __init__(self, words):
        h = [int(x) for x in words[:19]]
        (_, _, n_pub, cap, nz, nzo, n0, n_fri, fd, nq, w_wit, w_s2, w_q, w_su, depth, log_n, fri_lde, _, _) = h
        self.nq, self.cap, self.depth, self.sched = nq, cap, depth, [int(x) for x in words[19:19 + n_fri]]
        self.widths = (w_wit, w_s2, w_q, w_su)
        pos = 19 + n_fri
        self.ranges = {}

        def take(name, k):
            nonlocal pos
            self.ranges[name] = (pos, pos + k)
            pos += k
        take("public_inputs", n_pub)
        for name in ("witness_cap", "stage_2_cap", "quotient_cap"):
            take(name, cap * 4)
        take("values_at_z", 2 * nz)
        take("values_at_z_omega", 2 * nzo)
        take("values_at_0", 2 * n0)
        take("fri_caps", n_fri * cap * 4)
        take("final_monomials", 2 * fd)
        self.body = (19 + n_fri, len(words))
        self.query_start = pos
        self.index_words, self.query = [], []
        ln = (1 << log_n) * fri_lde
        for _ in range(nq):
            q = {}
            self.index_words.append(pos)
            pos += 1
            for name, w in (("witness", w_wit), ("stage_2", w_s2), ("quotient", w_q), ("setup", w_su)):
                q[name + "_leaf"] = (pos, pos + w)
                pos += w
                q[name + "_path"] = (pos, pos + 4 * depth)
                pos += 4 * depth
            l = ln
            for i, k in enumerate(self.sched):
                d = ((l >> k) // cap).bit_length() - 1
                q["fri%d_leaf" % i] = (pos, pos + (2 << k))
                pos += 2 << k
                q["fri%d_path" % i] = (pos, pos + 4 * d)
                pos += 4 * d
                l >>= k
            self.query.append(q)
        assert pos == len(words)
        self.indices = [int(words[p]) for p in self.index_words]      # the stored query indices: which slot of a FRI leaf is carried

    def classify(self, pos):
        for name, (a, b) in self.ranges.items():
            if a <= pos < b:
                return name
        for q in self.query:
            for name, (a, b) in q.items():
                if a <= pos < b:
                    return name
        return "index" if pos in self.index_words else None


SWEEP_CLASSES = ["witness_cap", "stage_2_cap", "quotient_cap", "values_at_z", "values_at_z_omega", "values_at_0", "fri_caps", "final_monomials",
                 "witness_leaf", "witness_path", "stage_2_leaf", "stage_2_path", "quotient_leaf", "quotient_path", "setup_leaf", "setup_path",
                 "fri1_leaf", "fri1_path"]


def sweep_positions(L, seed=20261018, count=300):
    """`count` positions of the body of a proof (everything behind header and schedule, the stored index words excluded) from one
    seeded generator: first two from every field class of SWEEP_CLASSES (the caps, opening groups and final monomials are a few
    words among thousands: a uniform draw misses them), the rest uniform over the body."""
    rng = np.random.default_rng(seed)
    out = []
    for name in SWEEP_CLASSES:
        spans = [L.ranges[name]] if name in L.ranges else [q[name] for q in L.query]
        for _ in range(2):
            a, b = spans[int(rng.integers(0, len(spans)))]
            out.append(int(rng.integers(a, b)))
    forbidden = set(L.index_words)
    while len(out) < count:
        pos = int(rng.integers(L.body[0], L.body[1]))
        if pos not in forbidden:
            out.append(pos)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# every word of a query: what each single-word edit must be rejected as (tests/test_gpu_verify_edges.py, tests/test_verify_edges_host.py)
# ---------------------------------------------------------------------------------------------------------------------------
from era_boojum_amd.binding import VERIFY_FRI_MERKLE, VERIFY_FRI_VALUE, VERIFY_MERKLE  # noqa: E402  (bj_verify_stage)

BASE_ORACLES = ("witness", "stage_2", "quotient", "setup")
# (transcript, tree_hasher) of ProverSetup -> transcript_kind of oracle.prover / oracle.verifier, hasher of oracle.prover.hashing_layer
# (None: the Poseidon (v1) trees of tests/poseidon1_layer.py, which the oracle takes through a patched hashing_layer)
PAIRINGS = [("poseidon2", None), ("poseidon", None), ("poseidon", "poseidon"), ("blake2s", None), ("keccak256", None)]
ORACLE_KIND = {("poseidon2", None): (1, 1), ("poseidon", None): (2, 1), ("poseidon", "poseidon"): (2, None), ("blake2s", None): (3, 2),
               ("keccak256", None): (4, 3)}
TREE_HASHER_PAIRINGS = [("poseidon2", None), ("poseidon", "poseidon"), ("blake2s", None), ("keccak256", None)]   # one per tree hasher


def oracle_layer(transcript, hasher):
    """(transcript_kind, the oracle's hashing layer) of a pairing: merkle_* / hash_leaf / hash_node / Transcript / QueryIndexer."""
    from oracle import prover as OP
    kind, h = ORACLE_KIND[(transcript, hasher)]
    if h is None:
        import poseidon1_layer as PL
        return kind, PL.poseidon1_layer(numpy_permutation=False)    # trees of 2^9 leaves: per-state C calls beat numpy's fixed cost
    return kind, OP.hashing_layer(h)


def oracle_verify(ovk, proof, transcript, hasher, monkeypatch, verbose=False):
    """oracle.verifier.verify under a pairing's transcript and tree hasher (verbose: it prints the check that failed)."""
    from oracle import prover as OP, verifier as OV
    kind, layer = oracle_layer(transcript, hasher)
    with monkeypatch.context() as m:
        m.setattr(OP, "hashing_layer", lambda _hasher: layer)
        return OV.verify(ovk, proof, verbose=verbose, transcript_kind=kind)


def drawn_indices(c, cap, proof, log_n, fri_lde, transcript="poseidon2", hasher=None):
    """Replays the oracle's transcript up to the query indices (oracle/verifier.py, no proof of work): the oracle prover's dict
    carries no stored indices (the reference's Proof has none)."""
    kind, H = oracle_layer(transcript, hasher)
    t = H.Transcript(kind)
    t.absorb_cap(cap)
    t.absorb(proof["public_inputs"])
    t.absorb_cap(np.array(proof["witness_oracle_cap"], dtype=np.uint64))
    for _ in range(4 if c.lookup_reps else 2):
        t.challenge_ext()
    t.absorb_cap(np.array(proof["stage_2_oracle_cap"], dtype=np.uint64))
    t.challenge_ext()
    t.absorb_cap(np.array(proof["quotient_oracle_cap"], dtype=np.uint64))
    t.challenge_ext()
    for grp in ("values_at_z", "values_at_z_omega", "values_at_0"):
        for v in proof[grp]:
            t.absorb(v)
    t.challenge_ext()
    for cap_ in [proof["fri_base_oracle_cap"]] + proof["fri_intermediate_oracles_caps"]:
        t.absorb_cap(np.array(cap_, dtype=np.uint64))
        t.challenge_ext()
    t.absorb(proof["final_fri_monomials"][0])
    t.absorb(proof["final_fri_monomials"][1])
    qi = H.QueryIndexer(log_n, fri_lde.bit_length() - 1)
    return [qi.next(t) for _ in proof["queries_per_fri_repetition"]]


def query_of(L, pos):
    """The query whose block (index word, openings) holds word `pos`, or None in front of the query section."""
    if pos < L.query_start:
        return None
    return max(q for q, first in enumerate(L.index_words) if first <= pos)


def carried_words(L, q, layer):
    """The two words (c0, c1) of FRI layer `layer`'s leaf of query q that hold the value carried into the layer: element `sub` of
    the leaf, sub = the low schedule[layer] bits of the query index once the earlier layers' bits are shifted out."""
    k = L.sched[layer]
    sub = (L.indices[q] >> sum(L.sched[:layer])) & ((1 << k) - 1)
    a = L.query[q]["fri%d_leaf" % layer][0]
    return a + sub, a + (1 << k) + sub


def expected_rejection(L, pos):
    """(stages, query, oracle) a proof with word `pos` of a query's openings edited must be rejected with, from the field class
    of the word (Layout.classify) and the order include/boojum_hip.h documents for bj_verify: the smallest failing query, inside
    it the four base oracles, then per FRI layer the carried value and then the layer's path.  `stages` holds ONE stage.  An
    edited leaf word of FRI layer l leaves every earlier check alone (the fold out of layer l is only compared at layer l + 1);
    at layer l the carried value is judged first, so it is FRI_VALUE for the two words of the carried slot and FRI_MERKLE (the
    leaf hash no longer leads to the cap) for every other one.  queries_checked is the query.  None for a word outside the
    openings (header, caps, evaluations, an index word)."""
    name, q = L.classify(pos), query_of(L, pos)
    if name is None or q is None or name == "index":
        return None
    for o, base in enumerate(BASE_ORACLES):
        if name in (base + "_leaf", base + "_path"):
            return {VERIFY_MERKLE}, q, o
    assert name.startswith("fri")
    layer = int(name[3:name.index("_")])
    if name.endswith("_path"):
        return {VERIFY_FRI_MERKLE}, q, layer
    return ({VERIFY_FRI_VALUE} if pos in carried_words(L, q, layer) else {VERIFY_FRI_MERKLE}), q, layer


def query_edit_batch(buf, L, q):
    """(positions, proofs): one `bump`ed copy of buf per word of query q's block — every leaf word and every path word of the four
    base oracles and of every FRI layer; the stored index word in front of them is left out."""
    end = L.index_words[q + 1] if q + 1 < L.nq else len(buf)
    positions = list(range(L.index_words[q] + 1, end))
    return positions, [bump(buf, pos) for pos in positions]


def fri_value_edit(buf, L, layer, query=0, H=None):
    """The carried slot (its c0 word) of `query`'s layer-`layer` leaf changed, the path walked again with the tree hasher H (hash_leaf /
    hash_node; default the oracle's Poseidon2) and the cap entry it ends at replaced: the layer's path verifies, the value
    folded out of the layer before it (layer 0: the DEEP value) is no longer in the leaf."""
    if H is None:
        import oracle as H
    words = np.array(buf, copy=True)
    q = L.query[query]
    tree = (L.indices[query] >> sum(L.sched[:layer])) >> L.sched[layer]
    a, b = q["fri%d_leaf" % layer]
    words = bump(words, carried_words(L, query, layer)[0])
    cur = H.hash_leaf(words[a:b])
    pa, pb = q["fri%d_path" % layer]
    for j in range((pb - pa) // 4):
        sib = words[pa + 4 * j: pa + 4 * j + 4]
        cur = H.hash_node(cur, sib) if tree % 2 == 0 else H.hash_node(sib, cur)
        tree //= 2
    cap0 = L.ranges["fri_caps"][0] + layer * L.cap * 4 + 4 * tree
    words[cap0:cap0 + 4] = cur
    return words


def query_moved_to_front(buf, L, q):
    """buf with the blocks (index word, openings) of query 0 and query q exchanged.  The openings are still the prover's, at the
    indices stored with them, but in slots whose drawn index is another one."""
    words = np.array(buf, copy=True)
    size = L.index_words[1] - L.index_words[0]
    a, b = L.index_words[0], L.index_words[q]
    words[a:a + size], words[b:b + size] = buf[b:b + size], buf[a:a + size]
    return words


# witness-leaf width -> (boolean_columns, num_witness_cols) on top of the SHA bench geometry (60 general-purpose + 8 x 4 lookup
# columns + multiplicities = 93 words): V = 92 + boolean_columns variable columns, leaf = V + num_witness_cols + 1.  The split
# steers the other oracles: stage 2 = 2 * ceil(V / 4) + 18 words, setup = V + 8 constants + 5 table words, quotient = 8.
#       W: (bc, wc)      stage 2 (mod 8, mod 17)   setup (mod 8, mod 17)
WITNESS_WIDTH_KNOBS = {
    96: (0, 3),        # 64 (0, 13)                105 (1, 3)
    97: (0, 4),        # 64 (0, 13)                105 (1, 3)
    102: (7, 2),       # 68 (4, 0)                 112 (0, 10)
    103: (8, 2),       # 68 (4, 0)                 113 (1, 11)
    119: (13, 13),     # 72 (0, 4)                 118 (6, 16)
    135: (37, 5),      # 84 (4, 16)                142 (6, 6)
    136: (31, 12),     # 80 (0, 12)                136 (0, 0)
}
EDGE_WIDTHS = sorted(WITNESS_WIDTH_KNOBS)


def oracle_widths(c):
    """Leaf widths (witness, stage 2, quotient, setup) a proof of circuit c has (oracle/verifier.py: wl, s2l, 2 * q, sul)."""
    V, q = c.num_vars, c.quotient_degree
    lookups = 1 if c.lookup_reps else 0
    return (V + c.num_witness_cols + lookups, 2 * ((V + q - 1) // q) + 2 * (c.lookup_reps + 1) * lookups, 2 * q,
            V + c.num_constant_cols + (c.lookup_width + 1) * lookups)


def circuit_with_witness_width(W, log_n, seed=31):
    """A satisfiable synthetic circuit (lookups on) whose witness-oracle leaf is exactly W words wide (header word 10 of its
    proofs), W >= 93: the SHA bench geometry plus Boolean specialized columns and unconstrained non-copiable witness columns
    (WITNESS_WIDTH_KNOBS; any other width: witness columns alone)."""
    assert W >= 93, W
    bc, wc = WITNESS_WIDTH_KNOBS.get(W, (0, W - 93))
    c = S.sha_shaped_circuit(log_n, seed=seed + W, table_bits=1 if log_n < 8 else 2, boolean_columns=bc, num_witness_cols=wc)
    assert c.lookup_reps and oracle_widths(c)[0] == W, (W, oracle_widths(c))
    return c
