"""era_boojum_amd/_abi.py — the generated ctypes view of include/boojum_hip.h every GPU test calls through — against the host C
compiler: a C program generated from the parsed header prints the size of every struct, the offset and size of every field, the
value of every enumerator and #define and the size of every scalar type a function takes or returns; ctypes must agree on all of
them.  A field added to the header only, a c_uint for a size_t or a renumbered enumerator fails here, on the CPU, not as a
corrupted argument in a process that has the GPU open.  (Signatures: tests/test_rust_bindings.py.)"""
import ctypes as C
import importlib.util
import os
import subprocess

from era_boojum_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# restated here, not read from the emitter
SCALAR_CLASS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "size_t": C.c_size_t, "uint64_t": C.c_uint64,
                "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}


def _header():
    spec = importlib.util.spec_from_file_location("abi_header", os.path.join(ROOT, "tools", "abi_header.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.parse_header()


def _scalars(h):
    """Every named enum, and every scalar type a function of the header takes or returns by value."""
    used = list(h["enums"])
    for _, ret, ps in h["funcs"]:
        for t in [ret] + [t for _, t in ps]:
            if not t.consts and t.base != "void" and t.base not in dict(h["fn_types"]) and t.base not in used:
                used.append(t.base)
    return used


def _probe_source(h):
    o = ["#include <stddef.h>", "#include <stdio.h>", '#include "boojum_hip.h"', "int main(void) {"]
    for name, fields in h["structs"]:
        o.append('    printf("struct|%s|%%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in fields:
            o.append('    printf("field|%s.%s|%%zu|%%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    for k, _ in h["defines"] + h["enum_consts"]:
        o.append('    printf("const|%s|%%lld\\n", (long long)%s);' % (k, k))
    for t in _scalars(h):
        o.append('    printf("scalar|%s|%%zu\\n", sizeof(%s));' % (t, t))
    return "\n".join(o + ["    return 0;", "}", ""])


def test_structs_constants_and_scalars_have_the_compilers_layout(tmp_path):
    h = _header()
    assert len(h["structs"]) == 11 and len(h["enum_consts"]) == 68 and len(h["defines"]) == 15
    src, exe = str(tmp_path / "abi_probe.c"), str(tmp_path / "abi_probe")
    with open(src, "w") as f:
        f.write(_probe_source(h))
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    lines = [ln.split("|") for ln in subprocess.check_output([exe], text=True).splitlines()]
    want_structs = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "struct"}
    want_fields = {ln[1]: (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "field"}
    want_consts = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "const"}
    want_scalars = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "scalar"}
    assert len(want_structs) == 11 and len(want_consts) == 68 + 15

    seen = 0
    for name, fields in h["structs"]:
        S = getattr(_abi, name)
        assert issubclass(S, C.Structure) and C.sizeof(S) == want_structs[name], name
        assert [f for f, _ in S._fields_] == [f for f, _ in fields], name        # header order, nothing more, nothing less
        for f, _ in fields:
            d = getattr(S, f)
            assert (d.offset, d.size) == want_fields["%s.%s" % (name, f)], (name, f)
            seen += 1
    assert seen == len(want_fields) > 11
    for k, v in want_consts.items():
        assert getattr(_abi, k) == v, k
    enums = set(h["enums"])
    assert enums and enums < set(want_scalars)
    for t, size in want_scalars.items():
        assert C.sizeof(C.c_int if t in enums else SCALAR_CLASS[t]) == size, t


def test_binding_names_are_the_generated_classes():
    """The names the binding, the tests and the tools use are aliases of the generated classes and constants, not copies."""
    from era_boojum_amd import binding as B, gate_program as G, synthetic as S
    assert (B.DeepSet, B._GateDesc, B._Circuit, B._ProofConfig, B._Comm) == (
        _abi.bj_deep_set, _abi.bj_gate_desc, _abi.bj_circuit, _abi.bj_proof_config, _abi.bj_comm)
    assert (B._VerifyReport, B._UnsatReport, B._CopyReport) == (_abi.bj_verify_report, _abi.bj_unsat_report, _abi.bj_copy_report)
    assert (G._GateIndex, G._GateRelation, G._GateProgram) == (_abi.bj_gate_index, _abi.bj_gate_relation, _abi.bj_gate_program)
    assert dict(_abi.bj_comm._fields_)["all_gather"] is B._ALL_GATHER_FN and dict(_abi.bj_comm._fields_)["all_gather_stream"] is B._ALL_GATHER_STREAM_FN
    assert _abi.SIGNATURES["bj_comm_peer_create"][1][2] is B._HOST_EXCHANGE_FN is _abi.bj_host_exchange_fn
    assert (B.ABI_VERSION, B.RCCL_UNIQUE_ID_BYTES, B.VERIFY_PARTIAL_QUERIES) == (6, 128, 1)
    assert (B.VERIFY_OK, B.VERIFY_FINAL, B.SAT, B.UNSAT_MULTIPLICITY, B.COPY_OK, B.COPY_VALUE_MISMATCH) == (0, 8, 0, 4, 0, 3)
    assert (S.GATE_CONSTANT_ALLOCATOR, S.GATE_FMA, S.GATE_REDUCTION4, S.GATE_NOP, S.GATE_PROGRAM, S.GATE_POSEIDON2_FLATTENED,
            S.GATE_POSEIDON_FLATTENED, S.TABLE_ID_AS_VARIABLE) == (1, 2, 3, 4, 5, 6, 7, 0xFFFFFFFF)
    assert (G.OP_ADD, G.OP_DOUBLE, G.OP_SUB, G.OP_NEGATE, G.OP_MUL, G.OP_SQUARE, G.OP_INVERSE) == (1, 2, 3, 4, 5, 6, 7)
    assert (G.IDX_VARIABLE, G.IDX_WITNESS, G.IDX_CONSTANT_POLY, G.IDX_TEMPORARY, G.IDX_VALUE) == (0, 1, 2, 3, 4)
    assert B.Context.FIELD_OPS["add"] == 0 and B.Context.FIELD_OPS["acc_ext2"] == 14 and B.Context.FIELD_OPS["w16_butterfly"] == 32 \
        and len(B.Context.FIELD_OPS) == 25
    cfg = B.proof_config_struct(8, 16, 100, 0, transcript="keccak256", pow_runner="keccak256")
    assert (cfg.transcript, cfg.tree_hasher, cfg.pow_runner) == (4, 3, 2)
    cfg = B.proof_config_struct(8, 16, 100, 0, transcript="poseidon", tree_hasher="poseidon")
    assert (cfg.fri_lde_factor, cfg.cap_size, cfg.security_level, cfg.pow_bits, cfg.transcript, cfg.tree_hasher, cfg.pow_runner) == (8, 16, 100, 0, 2, 4, 1)
