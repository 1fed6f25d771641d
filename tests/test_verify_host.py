"""CPU-side checks of the verifier's host layer: proof_format.serialize is the inverse of the parser, and bj_vk_create — which
needs no device — accepts the test circuits and refuses what bj_setup_create refuses, with a message."""
import ctypes as C
import types

import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, proof_format, synthetic as S
from verify_util import drawn_indices, golden_circuit, golden_config, golden_proof_dict


def test_serialize_round_trips_an_oracle_prover_proof():
    from oracle import prover as OP
    c = S.sha_shaped_circuit(8, seed=5, table_bits=2)
    setup = OP.Setup(c, 4, 8, threads=2)
    proof = OP.prove(c, setup, 4, 8, security_level=20, threads=2)
    # the oracle prover's dict carries no stored indices (the reference's Proof has none): draw them as its verifier does
    proof["_query_indices"] = drawn_indices(c, np.asarray(setup.cap), proof, 8, 4)
    words = proof_format.serialize(proof)
    back = proof_format.parse(words, security_level=20)
    for k, v in back.items():
        if k in ("proof_config", "_schedule"):
            continue
        assert _plain(proof[k]) == _plain(v), k
    assert back["proof_config"]["fri_lde_factor"] == 4 and back["proof_config"]["merkle_tree_cap_size"] == 8
    assert np.array_equal(proof_format.serialize(back), words)
    assert int(words[15]) == 8        # log_n derived from the path depth


def test_serialize_round_trips_the_golden_dict(fixture_json):
    fx = fixture_json
    g = golden_proof_dict(fx)
    g["_query_indices"] = list(range(len(g["queries_per_fri_repetition"])))
    words = proof_format.serialize(g)
    back = proof_format.parse(words)
    for k in ("public_inputs", "witness_oracle_cap", "stage_2_oracle_cap", "quotient_oracle_cap", "values_at_z", "values_at_z_omega",
              "values_at_0", "fri_base_oracle_cap", "fri_intermediate_oracles_caps", "final_fri_monomials", "queries_per_fri_repetition"):
        assert _plain(back[k]) == _plain(g[k]), k
    assert back["pow_challenge"] == int(g["pow_challenge"] or 0)
    assert int(words[15]) == fx["geometry"]["domain_size"].bit_length() - 1 and int(words[9]) == 6
    assert np.array_equal(proof_format.serialize(back), words)


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple, np.ndarray)):
        return [_plain(v) for v in x]
    return int(x) if x is not None else None


CONFIG = dict(fri_lde_factor=8, cap_size=16, security_level=20, pow_bits=0)


def _cap(cap_size=16):
    return np.arange(4 * cap_size, dtype=np.uint64)


@pytest.mark.parametrize("make", [
    lambda: S.sha_shaped_circuit(9, seed=3, table_bits=2),
    lambda: S.sha_shaped_circuit(9, seed=3, table_bits=2, table_id_as_variable=True),
    lambda: S.recursion_like_circuit(8, seed=2),
    lambda: S.recursion_like_circuit(8, seed=2, poseidon2_as_op_list=True),
    lambda: S.recursion_like_circuit(8, seed=2, poseidon1="kind"),
    lambda: S.recursion_like_circuit(8, seed=2, poseidon1=8),
    lambda: S.sha_shaped_circuit(9, seed=3, table_bits=2, gates=S.witness_gates(60, 4, 5), mix=(0.05, 0.3, 0.3, 0.2), num_witness_cols=5),
    lambda: S.sha_shaped_circuit(9, seed=3, table_bits=2, gates=S.host_gates(), mix=(0.05, 0.3, 0.3, 0.2)),
], ids=["sha", "sha_tid_var", "recursion", "recursion_p2_op_list", "recursion_p1_kind", "recursion_p1_witness", "witness_gates", "host_gates"])
def test_vk_create_accepts_the_test_circuits_without_a_device(make):
    vk = B.Verifier(make(), _cap(), CONFIG)
    vk.close()


def test_vk_create_accepts_the_golden_circuit(fixture_json):
    fx = fixture_json
    for with_gate in (True, False):
        B.Verifier(golden_circuit(fx, with_gate), np.array(fx["setup_merkle_tree_cap"], dtype=np.uint64), golden_config(fx)).close()


def _refused(circuit, config=CONFIG, cap=None):
    with pytest.raises(B.BoojumHipError) as e:
        B.Verifier(circuit, _cap(config["cap_size"]) if cap is None else cap, config)
    msg = str(e.value)
    assert "(-1)" in msg, msg                   # BJ_ERR_INVALID_ARG
    assert "null context" not in msg and len(msg.split(": ", 1)[1]) > 10, msg
    return msg


def test_vk_create_refuses_what_the_prover_refuses():
    c = S.sha_shaped_circuit(9, seed=3, table_bits=2)
    # 17 gate types
    many = types.SimpleNamespace(**{k: getattr(c, k) for k in ("log_n", "num_vars", "num_gp_vars", "num_witness_cols", "num_constant_cols",
                                                               "lookup_width", "lookup_reps", "table_id_col", "quotient_degree", "non_residues",
                                                               "public_inputs", "specialized_gates")})
    many.gates = list(c.gates) + [c.gates[-1]] * (17 - len(c.gates))
    assert "gates" in _refused(many)
    # a 9-bit selector path (bj_gate_desc.path holds 8 entries: the length alone is out of range)
    import copy
    long_path = copy.copy(many)
    long_path.gates = [copy.copy(g) for g in c.gates]
    long_path.gates[1].path = [True] * 9
    assert "bad gate descriptor 1" in _refused(long_path)
    # an op list that uses a temporary nothing wrote
    from era_boojum_amd import gate_program as GP
    e = S.sha_shaped_circuit(9, seed=3, table_bits=2, extended=True)
    bad = copy.copy(many)
    bad.gates = [copy.copy(g) for g in e.gates]
    bad.num_constant_cols, bad.table_id_col, bad.quotient_degree = e.num_constant_cols, e.table_id_col, e.quotient_degree
    i = next(k for k, g in enumerate(bad.gates) if g.name == "SelectionGate")
    good = bad.gates[i].program
    rel = list(good.relations)
    op, dst, a, b = rel[0]
    rel[0] = (op, dst, (3, good.num_temporaries + 5), b)
    bad.gates[i].program = GP.GateProgram(rel, list(good.values), list(good.writes), good.num_temporaries + 8)
    msg = _refused(bad)
    assert "operand in relation 0" in msg, msg      # the canonicaliser's words for it (csrc/gate_canon.cpp)
    # an unknown hasher pairing: a byte transcript with an algebraic tree hasher
    msg = _refused(c, dict(CONFIG, transcript="blake2s", tree_hasher="poseidon2"))
    assert "byte tree hasher" in msg, msg
