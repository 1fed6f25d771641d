"""The Rust side of the boundary is shipped as source (no Rust toolchain in the build image): rust/boojum_hip_sys.rs is GENERATED
from include/boojum_hip.h and must cover every entry point; the ctypes table the GPU tests call through (generated from the same
parse, era_boojum_amd/_abi.py) must give every parameter of every entry point its C type; rust/prove_hip.rs (the `prove_hip` sibling of
`prove_cpu_basic` + the BJPF -> `Proof` deserialiser) must be complete source that only uses symbols the header declares."""
import ctypes as C
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_rust_bindings", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# C scalar type -> the one ctypes class a parameter or a return value of that type may have (restated here, not read from the emitter)
SCALAR_CLASS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "size_t": C.c_size_t, "uint64_t": C.c_uint64,
                "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}


def _check_type(t, got, h, abi, what):
    """`got`, the restype or one argtype of the ctypes table, against the declaration `t` of the header."""
    if t.base in dict(h["fn_types"]) and not t.consts:       # a callback passed by value: its own CFUNCTYPE
        assert got is getattr(abi, t.base) and issubclass(got, C._CFuncPtr), what
    elif t.consts:                                           # a pointer: a pointer-class type, the string class for `char *` only
        assert got in (C.c_void_p, C.c_char_p), what
        assert (got is C.c_char_p) == (t.base == "char" and len(t.consts) == 1), what
    elif t.base == "void":
        assert got is None, what
    else:
        assert got is (C.c_int if t.base in h["enums"] else SCALAR_CLASS[t.base]), what


def test_generated_bindings_are_current_and_cover_the_header():
    g = _gen()
    committed = open(os.path.join(ROOT, "rust", "boojum_hip_sys.rs")).read()
    assert g.generate() == committed, "rust/boojum_hip_sys.rs is stale: run python tools/gen_rust_bindings.py"
    h = g.parse_header()
    from era_boojum_amd import binding
    from era_boojum_amd import _abi
    rust_fns = {name: len(ps) for name, _, ps in h["funcs"]}
    assert set(rust_fns) == set(binding._SIGNATURES), set(rust_fns) ^ set(binding._SIGNATURES)
    assert binding._SIGNATURES is _abi.SIGNATURES
    for name, ret, ps in h["funcs"]:        # the ctypes table the GPU tests call through: arity, every parameter's type, the result's
        res, args = binding._SIGNATURES[name]
        assert rust_fns[name] == len(args), name
        _check_type(ret, res, h, _abi, name)
        for (pname, t), got in zip(ps, args):
            _check_type(t, got, h, _abi, "%s(%s)" % (name, pname))
    structs = dict(h["structs"])
    assert [f for f, _ in structs["bj_comm"]] == ["rank", "world", "all_gather", "user", "all_gather_stream"]
    assert [f for f, _ in structs["bj_circuit"]][:4] == ["log_n", "num_vars", "num_gp_vars", "num_witness_cols"]
    assert "pub path: [u8; 8]," in committed and "Option<unsafe extern \"C\" fn(" in committed


def test_prove_hip_source_is_complete():
    src = open(os.path.join(ROOT, "rust", "prove_hip.rs")).read()
    assert "unimplemented!" not in src and "todo!" not in src
    for needed in ("pub fn prove_hip<", "pub fn hip_setup<", "pub fn proof_from_bjpf<", "fn from_capture(", "bj_setup_create_sharded(", "bj_prove(",
                   "bj_proof_serialize(", "queries_per_fri_repetition", "fri_intermediate_oracles_caps", "pow_challenge"):
        assert needed in src, needed
    declared = set(re.findall(r"pub fn (bj_[a-z0-9_]+)", open(os.path.join(ROOT, "rust", "boojum_hip_sys.rs")).read()))
    used = set(re.findall(r"\b(bj_[a-z0-9_]+)\(", src))
    assert used <= declared, used - declared
    # the deserialiser reads the header fields the serialiser writes (csrc/prover.hip) in the same order as proof_format.py
    from era_boojum_amd import proof_format
    assert "0x424A_5046" in src and proof_format.MAGIC == 0x424A5046


def test_array_parameters_decay_to_pointers_and_array_fields_stay_arrays():
    """C adjusts a parameter `uint64_t fp[2]` to `uint64_t *fp`: the binding must pass one address, not 16 bytes by value
    (ADVICE round 3); a struct field `unsigned char path[8]` stays an inline array."""
    g = _gen()
    h = g.parse_header()

    def rust(decl):
        return decl[0], g.rust_type(decl[1], h)
    assert rust(g.parse_param("uint64_t fp[2]", decay=True)) == ("fp", "*mut u64")
    assert rust(g.parse_param("const uint64_t roots[4]", decay=True)) == ("roots", "*const u64")
    assert rust(g.parse_param("uint32_t v[]", decay=True)) == ("v", "*mut u32")
    assert rust(g.parse_param("unsigned char path[8]")) == ("path", "[u8; 8]")
    funcs = {name: [rust(p) for p in ps] for name, _, ps in h["funcs"]}
    assert dict(funcs["bj_gate_program_canonical_info"])["fp"] == "*mut u64"
    for name, ps in funcs.items():
        assert not any(t.startswith("[") for _, t in ps), name        # no by-value array in any extern "C" signature
    from era_boojum_amd import _abi                                    # nor in the ctypes table: one address
    assert _abi.SIGNATURES["bj_gate_program_canonical_info"][1][1] is C.c_void_p
