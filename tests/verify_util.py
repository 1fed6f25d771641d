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
