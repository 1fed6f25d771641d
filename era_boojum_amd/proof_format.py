"""Parser (and its inverse) of the flat u64 proof serialisation produced by bj_proof_serialize (csrc/prover.hip) into a dict with the field
names of the reference's `Proof` (src/cs/implementations/proof.rs:121-136).

Layout (all u64, little endian; the definition of the word order is csrc/proof_layout.h — bj::ProofHeader and bj::SerialLayout, which
the prover writes through and the verifier reads through; this parser reads the header words, it does not derive them):
  header[19] = magic 'BJPF', version (2), n_public, cap_size, n_values_at_z, n_values_at_z_omega, n_values_at_0, n_fri_oracles,
               final_degree, n_queries, witness leaf width, stage-2 leaf width, quotient leaf width, setup leaf width,
               base-oracle path depth, log_n, fri_lde_factor, pow_bits, pow_challenge      (version 1: the first 17 only)
  schedule[n_fri_oracles] | public inputs | witness cap | stage-2 cap | quotient cap (cap_size*4 each)
  values_at_z (2 each) | values_at_z_omega | values_at_0 | FRI caps (n_fri_oracles * cap_size*4)
  final monomials c0[final_degree], c1[final_degree]
  per query: index | for each of {witness, stage-2, quotient, setup}: leaf elements, path (depth*4)
             | for each FRI oracle i: 2*2^schedule[i] leaf elements, path
"""
import numpy as np

MAGIC = 0x424A5046


def parse(buf, security_level=None, pow_bits=0):
    a = np.asarray(buf, dtype=np.uint64)
    pos = 0

    def take(k):
        nonlocal pos
        out = a[pos:pos + k]
        if out.size != k:
            raise ValueError("truncated proof buffer")
        pos += k
        return out

    h = [int(x) for x in take(17)]
    if h[0] != MAGIC or h[1] not in (1, 2):
        raise ValueError("not a BJPF v1/v2 proof")
    (_, version, n_pub, cap, nz, nzo, n0, n_fri, final_degree, n_queries, w_wit, w_s2, w_q, w_su, depth, log_n, fri_lde) = h
    pow_challenge = 0
    if version == 2:
        pow_bits, pow_challenge = (int(x) for x in take(2))
    sched = [int(x) for x in take(n_fri)]
    caps4 = lambda: take(cap * 4).reshape(cap, 4).tolist()
    pairs = lambda k: take(2 * k).reshape(k, 2).tolist()
    proof = {"proof_config": {"fri_lde_factor": fri_lde, "merkle_tree_cap_size": cap, "fri_folding_schedule": None,
                              "security_level": security_level, "pow_bits": pow_bits}}
    proof["public_inputs"] = take(n_pub).tolist()
    proof["witness_oracle_cap"] = caps4()
    proof["stage_2_oracle_cap"] = caps4()
    proof["quotient_oracle_cap"] = caps4()
    proof["values_at_z"] = pairs(nz)
    proof["values_at_z_omega"] = pairs(nzo)
    proof["values_at_0"] = pairs(n0)
    fri_caps = [caps4() for _ in range(n_fri)]
    proof["fri_base_oracle_cap"] = fri_caps[0]
    proof["fri_intermediate_oracles_caps"] = fri_caps[1:]
    proof["final_fri_monomials"] = [take(final_degree).tolist(), take(final_degree).tolist()]
    queries, indices = [], []
    n_leaves = (1 << log_n) * fri_lde
    for _ in range(n_queries):
        indices.append(int(take(1)[0]))
        qd = {}
        for name, w in (("witness_query", w_wit), ("stage_2_query", w_s2), ("quotient_query", w_q), ("setup_query", w_su)):
            qd[name] = {"leaf_elements": take(w).tolist(), "proof": take(depth * 4).reshape(depth, 4).tolist()}
        qd["fri_queries"] = []
        ln = n_leaves
        for k in sched:
            d = ((ln >> k) // cap).bit_length() - 1
            qd["fri_queries"].append({"leaf_elements": take(2 << k).tolist(), "proof": take(d * 4).reshape(d, 4).tolist()})
            ln >>= k
        queries.append(qd)
    if pos != a.size:
        raise ValueError("trailing data in proof buffer")
    proof["queries_per_fri_repetition"] = queries
    proof["pow_challenge"] = pow_challenge
    proof["_query_indices"] = indices
    proof["_schedule"] = sched
    return proof


def serialize(proof, log_n=None):
    """The inverse of `parse`: the BJPF version 2 words of a proof dict (parse(serialize(p)) == p up to the fields the words do not
    carry: security_level comes back as given to `parse`).  The header fields are derived from the dict — the leaf widths and the
    path depth from the first query, the schedule from `_schedule` or from the FRI leaf sizes, log_n from the depth unless given —
    so a dict cut out of the reference's `Proof` JSON (tests/golden) serialises as well as one that `parse` returned; a proof
    without queries needs log_n and serialises zero widths."""
    cfg = proof["proof_config"]
    cap, fri_lde = int(cfg["merkle_tree_cap_size"]), int(cfg["fri_lde_factor"])
    queries = proof["queries_per_fri_repetition"]
    fri_caps = [proof["fri_base_oracle_cap"]] + list(proof["fri_intermediate_oracles_caps"])
    names = ("witness_query", "stage_2_query", "quotient_query", "setup_query")
    if queries:
        q0 = queries[0]
        widths = [len(q0[k]["leaf_elements"]) for k in names]
        depth = len(q0["witness_query"]["proof"])
        sched = [int(k) for k in proof["_schedule"]] if "_schedule" in proof else [(len(f["leaf_elements"]) // 2).bit_length() - 1 for f in q0["fri_queries"]]
        if log_n is None:
            log_n = depth + cap.bit_length() - 1 - (fri_lde.bit_length() - 1)
    else:
        widths, depth, sched = [0, 0, 0, 0], 0, [int(k) for k in proof.get("_schedule", [])]
        if log_n is None:
            raise ValueError("a proof without queries does not tell its trace length: pass log_n")
    if len(sched) != len(fri_caps):
        raise ValueError("schedule and FRI caps disagree")
    fm = proof["final_fri_monomials"]
    indices = proof.get("_query_indices")
    if indices is None or len(indices) != len(queries):
        raise ValueError("_query_indices: one stored index per query is needed")
    out = [MAGIC, 2, len(proof["public_inputs"]), cap, len(proof["values_at_z"]), len(proof["values_at_z_omega"]), len(proof["values_at_0"]),
           len(fri_caps), len(fm[0]), len(queries)] + widths + [depth, int(log_n), fri_lde, int(cfg.get("pow_bits") or 0),
                                                                int(proof.get("pow_challenge") or 0)]
    out += sched
    out += [int(x) for x in proof["public_inputs"]]

    def flat(rows):
        return [int(x) for row in rows for x in row]
    for k in ("witness_oracle_cap", "stage_2_oracle_cap", "quotient_oracle_cap", "values_at_z", "values_at_z_omega", "values_at_0"):
        out += flat(proof[k])
    for c in fri_caps:
        out += flat(c)
    out += [int(x) for x in fm[0]] + [int(x) for x in fm[1]]
    for idx, qd in zip(indices, queries):
        out.append(int(idx))
        for k in names:
            out += [int(x) for x in qd[k]["leaf_elements"]] + flat(qd[k]["proof"])
        for f in qd["fri_queries"]:
            out += [int(x) for x in f["leaf_elements"]] + flat(f["proof"])
    return np.array(out, dtype=np.uint64)
