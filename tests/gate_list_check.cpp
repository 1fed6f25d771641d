// Stand-alone check of csrc/gate_list.h (tests/test_gate_list_host.py builds it with the address and undefined-behaviour
// sanitizers): bj::resolve_gates on circuits written out here, against numbers worked out by hand from the descriptors —
// first_term is the sum of repetitions x terms over the earlier gates of the category, the specialized variable columns follow
// general-purpose + lookup columns, the specialized constant columns are the last ones — and one refusal per check it makes.
#include "gate_list.h"

#include <cstdio>
#include <deque>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// an op list with given extents: it reads variable var_extent - 1, constant const_extent - 1 and witness wit_extent - 1 (each when
// the extent is not 0) and writes n_writes terms.  resolve_gates looks at nothing else of a program.
struct Prog {
    std::vector<bj_gate_relation> rel;
    std::vector<bj_gate_index> writes;
    bj_gate_program p{};
};
static std::deque<Prog> progs;
static const bj_gate_program *prog(unsigned var_extent, unsigned const_extent, unsigned wit_extent, unsigned n_writes) {
    progs.emplace_back();
    Prog &P = progs.back();
    uint32_t t = 0;
    auto read = [&](uint32_t kind, unsigned extent) {
        if (extent) P.rel.push_back({BJ_OP_DOUBLE, t++, {kind, extent - 1}, {0, 0}});
    };
    read(BJ_IDX_VARIABLE_POLY, var_extent);
    read(BJ_IDX_CONSTANT_POLY, const_extent);
    read(BJ_IDX_WITNESS_POLY, wit_extent);
    for (unsigned k = 0; k < n_writes; k++) P.writes.push_back({BJ_IDX_TEMPORARY, 0});
    P.p.relations = P.rel.data(); P.p.num_relations = (uint32_t)P.rel.size();
    P.p.writes = P.writes.data(); P.p.num_writes = n_writes;
    P.p.num_temporaries = t;
    return &P.p;
}

static bj_gate_desc gate(int kind, std::initializer_list<int> path, unsigned reps, unsigned var_stride, unsigned const_stride, unsigned num_terms,
                         const bj_gate_program *program = nullptr, unsigned wit_stride = 0) {
    bj_gate_desc G{};
    G.kind = kind;
    for (int b : path) {
        if (G.path_len < 8) G.path[G.path_len] = (unsigned char)b;
        G.path_len++;
    }
    G.num_repetitions = reps; G.var_stride = var_stride; G.const_stride = const_stride; G.wit_stride = wit_stride; G.num_terms = num_terms;
    G.program = program;
    return G;
}

struct Circuit {
    std::vector<bj_gate_desc> gates, spec;
    bj_circuit c{};
    unsigned lookup_cps = 0;
    const bj_circuit &view() {
        c.num_gates = (unsigned)gates.size(); c.gates = gates.data();
        c.num_specialized_gates = (unsigned)spec.size(); c.specialized_gates = spec.empty() ? nullptr : spec.data();
        return c;
    }
};

// the SHA-256 bench shape: 60 general-purpose columns, width-4 lookups x 8 with the table id in constant column 7
static Circuit sha_bench() {
    Circuit C;
    C.gates = {gate(BJ_GATE_CONSTANT_ALLOCATOR, {0, 0, 1}, 4, 1, 1, 1), gate(BJ_GATE_FMA_NO_CONSTANT, {1}, 15, 4, 0, 1),
               gate(BJ_GATE_REDUCTION4, {0, 1}, 12, 5, 0, 1), gate(BJ_GATE_NOP, {0, 0, 0}, 1, 0, 0, 0)};
    C.c.num_gp_vars = 60; C.c.num_vars = 92; C.c.num_constant_cols = 8; C.c.lookup_width = 4; C.c.lookup_reps = 8; C.c.table_id_col = 7;
    C.lookup_cps = 4;
    return C;
}

// the recursion-class shape (synthetic.recursion_gates(130, 8)): 130 general-purpose columns, width-3 lookups x 8, the Boolean
// gate over one specialized column.  Table id as constant column 11: 130 + 24 + 1 = 155 columns, 12 constant columns; table id
// as a variable: 130 + 32 + 1 = 163 columns, 11 constant columns.
static Circuit recursion_class(bool table_id_as_variable) {
    Circuit C;
    C.gates = {gate(BJ_GATE_CONSTANT_ALLOCATOR, {0, 0, 0}, 8, 1, 1, 1),
               gate(BJ_GATE_PROGRAM, {0, 1, 1, 0, 1, 1}, 5, 26, 0, 2, prog(26, 0, 0, 2)),      // U8x4FMAGate
               gate(BJ_GATE_POSEIDON2_FLATTENED, {1}, 1, 130, 0, 118),
               gate(BJ_GATE_PROGRAM, {0, 1, 1, 1, 0, 1}, 14, 9, 0, 1, prog(9, 0, 0, 1)),       // DotProductGate<4>
               gate(BJ_GATE_PROGRAM, {0, 1, 1, 1, 0, 0}, 43, 3, 0, 2, prog(3, 0, 0, 2)),       // ZeroCheckGate
               gate(BJ_GATE_FMA_NO_CONSTANT, {0, 1, 1, 1, 1}, 32, 4, 0, 1),
               gate(BJ_GATE_PROGRAM, {0, 1, 0}, 26, 5, 0, 2, prog(5, 1, 0, 2)),                // UIntXAddGate
               gate(BJ_GATE_PROGRAM, {0, 1, 1, 0, 0, 1}, 32, 4, 0, 1, prog(4, 0, 0, 1)),       // SelectionGate
               gate(BJ_GATE_PROGRAM, {0, 1, 1, 0, 1, 0}, 10, 13, 0, 4, prog(13, 0, 0, 4)),     // ParallelSelectionGate<4>
               gate(BJ_GATE_REDUCTION4, {0, 0, 1}, 26, 5, 0, 1),
               gate(BJ_GATE_NOP, {0, 1, 1, 0, 0, 0}, 1, 0, 0, 0)};
    C.spec = {gate(BJ_GATE_PROGRAM, {}, 1, 1, 0, 1, prog(1, 0, 0, 1))};                        // BooleanConstraintGate
    C.c.num_gp_vars = 130; C.c.lookup_width = 3; C.c.lookup_reps = 8;
    if (table_id_as_variable) {
        C.c.num_vars = 163; C.c.num_constant_cols = 11; C.c.table_id_col = BJ_TABLE_ID_AS_VARIABLE; C.lookup_cps = 4;
    } else {
        C.c.num_vars = 155; C.c.num_constant_cols = 12; C.c.table_id_col = 11; C.lookup_cps = 3;
    }
    return C;
}

// the SHA shape with two gates over specialized columns that read constants: 2 repetitions of 3 variables and 1 constant, then
// 3 repetitions of 1 variable and 2 constants.  Variables 60 + 32 + 6 + 3 = 101; constants 7 + table id + 2 + 6 = 16.
static Circuit two_specialized() {
    Circuit C = sha_bench();
    C.spec = {gate(BJ_GATE_PROGRAM, {}, 2, 3, 1, 2, prog(3, 1, 0, 2)), gate(BJ_GATE_PROGRAM, {}, 3, 1, 2, 1, prog(1, 2, 0, 1))};
    C.c.num_vars = 101; C.c.num_constant_cols = 16;
    return C;
}

static bj::GateList L;
static std::string err;
static int resolve(Circuit &C, const bj::GateProgramCheck &check = nullptr) { return bj::resolve_gates(C.view(), C.lookup_cps, &L, &err, check); }
static bool refused(Circuit &C, int code, const char *words) {
    const int rc = resolve(C);
    const bool ok = rc == code && err.find(words) != std::string::npos;
    if (!ok) std::printf("  got %d \"%s\", expected %d \"...%s...\"\n", rc, err.c_str(), code, words);
    return ok;
}

int main() {
    {   // gate_kind_extent, kinds 1..7: {variables, constants, constants per repetition, terms, one repetition}
        const struct { unsigned v, c; bool per_rep; unsigned terms; bool single; } want[8] = {
            {}, {1, 1, true, 1, false}, {4, 2, false, 1, false}, {5, 4, false, 1, false}, {0, 0, true, 0, false}, {0, 0, true, 0, false},
            {130, 0, true, 118, true}, {130, 0, true, 118, true}};
        for (int k = 1; k <= 7; k++) {
            const bj::GateKindExtent e = bj::gate_kind_extent(k);
            CHECK(e.var_extent == want[k].v && e.const_extent == want[k].c && e.fixed_terms == want[k].terms && e.single_rep == want[k].single);
            if (e.const_extent) CHECK(e.const_per_rep == want[k].per_rep);
        }
    }
    {   // SHA-256 bench: 4 + 15 + 12 terms, the NOP none
        Circuit C = sha_bench();
        CHECK(resolve(C) == BJ_OK && err.empty());
        CHECK(L.general.size() == 4 && L.spec.empty() && L.n_general_terms == 31 && L.n_spec_terms == 0);
        const unsigned first[4] = {0, 4, 19, 31}, terms[4] = {4, 15, 12, 0};
        for (size_t g = 0; g < L.general.size() && g < 4; g++) {
            CHECK(L.general[g].first_term == first[g] && L.general[g].terms() == terms[g]);
            CHECK(L.general[g].first_col == 0 && L.general[g].first_const == 0 && L.general[g].kind == (int)g + 1);
        }
        const bj::GateShape &ca = L.general[0];
        CHECK(ca.path_len == 3 && ca.path[0] == 0 && ca.path[1] == 0 && ca.path[2] == 1 && ca.reps == 4 && ca.var_stride == 1 && ca.const_stride == 1);
    }
    for (bool tid_var : {false, true}) {   // recursion class: eleven gates, 418 terms; the Boolean gate behind the lookup columns
        Circuit C = recursion_class(tid_var);
        CHECK(resolve(C) == BJ_OK);
        const unsigned first[11] = {0, 8, 18, 136, 150, 236, 268, 320, 352, 392, 418};
        CHECK(L.general.size() == 11 && L.n_general_terms == 418);
        for (size_t g = 0; g < L.general.size() && g < 11; g++) CHECK(L.general[g].first_term == first[g]);
        CHECK(L.general[10].terms() == 0 && L.general[2].terms() == 118 && L.general[4].terms() == 86);
        CHECK(L.spec.size() == 1 && L.n_spec_terms == 1);
        CHECK(L.spec[0].first_col == (tid_var ? 162u : 154u) && L.spec[0].first_const == (tid_var ? 11u : 12u) && L.spec[0].first_term == 0);
    }
    {   // two specialized gates: their constants are the last columns, right behind the table-id column 7
        Circuit C = two_specialized();
        CHECK(resolve(C) == BJ_OK);
        CHECK(L.spec.size() == 2 && L.n_spec_terms == 7 && L.n_general_terms == 31);
        CHECK(L.spec[0].first_col == 92 && L.spec[0].first_const == 8 && L.spec[0].first_term == 0 && L.spec[0].const_stride == 1);
        CHECK(L.spec[1].first_col == 98 && L.spec[1].first_const == 10 && L.spec[1].first_term == 4 && L.spec[1].const_stride == 2);
        C.c.num_constant_cols = 17;   // a column between the table id and theirs
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "17 constant columns declared; the specialized gates' 8 must be the last ones, right behind the table-id column"));
        C.c.num_constant_cols = 15;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "last ones, right behind the table-id column"));
    }
    // ---- one refusal per check ----
    {
        Circuit C = sha_bench();
        C.gates[1] = gate(BJ_GATE_FMA_NO_CONSTANT, {1, 0, 1, 0, 1, 0, 1}, 15, 4, 0, 1);   // path of 7
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 1"));
        C.gates[1] = gate(BJ_GATE_FMA_NO_CONSTANT, {1, 0, 1, 0, 1, 0}, 15, 4, 0, 1);      // 6 + 2 constants of 8: the longest that fits
        CHECK(resolve(C) == BJ_OK);
        C.gates[1] = gate(BJ_GATE_FMA_NO_CONSTANT, {1}, 15, 4, 0, 2);                      // a hand-written kind has one term
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 1"));
        C.gates[1] = gate(0, {1}, 15, 4, 0, 1);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 1"));
        C.gates[1] = gate(8, {1}, 15, 4, 0, 1);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 1"));
        C.gates[1] = gate(BJ_GATE_PROGRAM, {1}, 15, 4, 0, 1);                              // no program
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 1"));
    }
    for (int kind : {BJ_GATE_POSEIDON2_FLATTENED, BJ_GATE_POSEIDON_FLATTENED}) {   // flattened gates: 118 terms, one repetition, 130 columns
        Circuit C = recursion_class(false);
        C.gates[2] = gate(kind, {1}, 1, 130, 0, 118);
        CHECK(resolve(C) == BJ_OK);
        C.gates[2] = gate(kind, {1}, 1, 130, 0, 117);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 2"));
        C.gates[2] = gate(kind, {1}, 2, 130, 0, 118);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 2"));
        C.gates[2] = gate(kind, {1}, 1, 130, 0, 118);
        C.c.num_gp_vars = 129; C.c.num_vars = 154;
        C.gates[0] = gate(BJ_GATE_NOP, {0, 0, 0}, 1, 0, 0, 0);   // only the flattened gate is too wide for 129 columns
        C.gates[1] = C.gates[0];
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "bad gate descriptor 2"));
    }
    {   // a variable / constant column out of range by one
        Circuit C = sha_bench();
        C.c.num_gp_vars = 59; C.c.num_vars = 91;   // FMA repetition 14 reads columns 56..59
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 1 reads variable column 60 / constant column 3 of 59 / 8 "
                                              "(repetitions x stride + operand index, after a selector path of 1)"));
        C = sha_bench();
        C.gates[0] = gate(BJ_GATE_CONSTANT_ALLOCATOR, {0, 0, 1}, 6, 1, 1, 1);   // constants 3..8 of 8
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 0 reads variable column 6 / constant column 9 of 60 / 8"));
        C.gates[0] = gate(BJ_GATE_CONSTANT_ALLOCATOR, {0, 0, 1}, 5, 1, 1, 1);   // constants 3..7
        CHECK(resolve(C) == BJ_OK);
        C.gates[2] = gate(BJ_GATE_REDUCTION4, {0, 1, 0, 1, 0}, 12, 5, 0, 1);    // 5 + 4 shared constants of 8
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 2 reads variable column 60 / constant column 9 of 60 / 8"));
        C.gates[2] = gate(BJ_GATE_REDUCTION4, {0, 1}, 0, 5, 0, 1);              // no repetition
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 2 reads variable column"));
        C = sha_bench();
        C.gates[3] = gate(BJ_GATE_PROGRAM, {0, 0, 0}, 7, 9, 2, 1, prog(6, 2, 0, 1));   // variables to 6 * 9 + 6 = 60, constants to 3 + 6 * 2 + 2 = 17
        C.c.num_constant_cols = 17; C.c.table_id_col = 16;
        CHECK(resolve(C) == BJ_OK);
        C.gates[3].program = prog(7, 2, 0, 1);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 3 reads variable column 61 / constant column 17 of 60 / 17"));
        C.gates[3].program = prog(6, 3, 0, 1);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 3 reads variable column 60 / constant column 18 of 60 / 17"));
        // the entry point that is handed the columns says so in its own words
        bj::GateShape s;
        CHECK(bj::resolve_gate(C.gates[3], 3, {60, 17, 0}, &s, &err, "reads past the given columns") == BJ_ERR_INVALID_ARG &&
              err == "gate 3 reads past the given columns");
        C = sha_bench();
        C.gates[3] = gate(BJ_GATE_NOP, {0, 0, 0}, 1, 0, 0, 0);
        C.c.num_constant_cols = 2; C.c.table_id_col = 1;
        C.gates.erase(C.gates.begin(), C.gates.begin() + 3);
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 0: selector path longer than the constant columns"));
    }
    {   // a witness column out of range by one: 3 repetitions 2 apart, the last reads witness 2 * 2 + 1 = 5 -> 5 columns are needed
        Circuit C = sha_bench();
        C.gates[3] = gate(BJ_GATE_PROGRAM, {0, 0, 0}, 3, 4, 0, 1, prog(4, 0, 1, 1), 2);
        C.c.num_witness_cols = 5;
        CHECK(resolve(C) == BJ_OK && L.general[3].wit_stride == 2 && L.general[3].first_term == 31 && L.n_general_terms == 34);
        C.c.num_witness_cols = 4;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 3 reads witness column 5 of 4"));
    }
    {   // num_writes != num_terms
        Circuit C = sha_bench();
        C.gates[3] = gate(BJ_GATE_PROGRAM, {0, 0, 0}, 3, 4, 0, 3, prog(4, 0, 0, 2));
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 3: program writes 2 terms, descriptor says 3"));
    }
    {   // more than 16 gates
        Circuit C = sha_bench();
        C.gates.resize(17, gate(BJ_GATE_NOP, {0, 0, 0}, 1, 0, 0, 0));
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "17 gate types over general-purpose columns (at most 16)"));
    }
    {   // specialized gates: a selector path, shared constants, a witness column, a hand-written kind
        Circuit C = two_specialized();
        C.spec[0] = gate(BJ_GATE_PROGRAM, {1}, 2, 3, 1, 2, prog(3, 1, 0, 2));
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "specialized gate 0 must be an op list without a selector path"));
        C = two_specialized();
        C.spec[1] = gate(BJ_GATE_PROGRAM, {}, 3, 1, 0, 1, prog(1, 2, 0, 1));   // reads constants, const_stride 0: shared
        C.c.num_constant_cols = 10;
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "specialized gate 1 must be an op list") && err.find("(share_constants = false)") != std::string::npos);
        C = two_specialized();
        C.spec[1].program = prog(1, 2, 1, 1);
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "specialized gate 1 must be an op list") && err.find("no witness column") != std::string::npos);
        C.spec[1].program = prog(2, 2, 0, 1);   // reads the next repetition's variable
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "specialized gate 1 must be an op list"));
        C.spec[1].program = prog(1, 2, 0, 2);   // writes two terms, declares one
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "specialized gate 1 must be an op list"));
        C = two_specialized();
        C.spec[0] = gate(BJ_GATE_FMA_NO_CONSTANT, {}, 2, 3, 1, 2);
        CHECK(refused(C, BJ_ERR_UNSUPPORTED, "specialized gate 0 must be an op list"));
    }
    {   // the column total off by one, either way
        Circuit C = two_specialized();
        C.c.num_vars = 102;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "102 variable columns declared, geometry + lookups + specialized gates make 101"));
        C.c.num_vars = 100;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "specialized gate 1 runs past the 100 declared variable columns"));
        C = sha_bench();
        C.c.num_vars = 93;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "93 variable columns declared, geometry + lookups + specialized gates make 92"));
    }
    {   // repetitions x stride that wrap 32 bits: 2^31 x 2
        Circuit C = two_specialized();
        C.spec[1] = gate(BJ_GATE_PROGRAM, {}, 0x80000000u, 2, 0, 1, prog(1, 0, 0, 1));   // 2^32 variable columns, 0 when wrapped
        C.c.num_constant_cols = 10; C.c.num_vars = 98;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "specialized gate 1 runs past the 98 declared variable columns"));
        C = two_specialized();
        C.spec[1] = gate(BJ_GATE_PROGRAM, {}, 0x80000000u, 1, 2, 1, prog(1, 2, 0, 1));   // 2^32 constant columns
        C.c.num_constant_cols = 10;
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "constant columns declared; the specialized gates'"));
        C = sha_bench();
        C.gates[1] = gate(BJ_GATE_FMA_NO_CONSTANT, {1}, 0x40000001u, 4, 0, 1);           // (2^30) x 4 + 4 = 2^32 + 4
        CHECK(refused(C, BJ_ERR_INVALID_ARG, "gate 1 reads variable column 4294967300 /"));
    }
    {   // the op-list check runs once per op list, where that list has passed every other check on its gate; its status comes
        // back as it is, with no message of this header's
        Circuit C = recursion_class(false);
        std::vector<const bj_gate_program *> seen;
        CHECK(resolve(C, [&](const bj_gate_program *p) { seen.push_back(p); return 0; }) == BJ_OK);
        CHECK(seen.size() == 7 && seen[0] == C.gates[1].program && seen[5] == C.gates[8].program && seen[6] == C.spec[0].program);
        int calls = 0;
        CHECK(resolve(C, [&](const bj_gate_program *) { return ++calls == 3 ? -5 : 0; }) == -5 && err.empty() && calls == 3);
        C.gates[4].num_terms = 3;   // gate 4 is refused before its list is looked at, after the lists of gates 1 and 3
        seen.clear();
        CHECK(resolve(C, [&](const bj_gate_program *p) { seen.push_back(p); return 0; }) == BJ_ERR_INVALID_ARG && seen.size() == 2);
        C = recursion_class(false);
        C.c.num_vars = 154;         // the specialized gate's list is looked at before its columns are counted
        seen.clear();
        CHECK(resolve(C, [&](const bj_gate_program *p) { seen.push_back(p); return 0; }) == BJ_ERR_INVALID_ARG && seen.size() == 7 &&
              err.find("runs past") != std::string::npos);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("gate list == expected\n");
    return 0;
}
