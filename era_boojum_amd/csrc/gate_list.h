// The circuit's gates, resolved once: every consumer of a gate list (setup, prover, satisfiability check, verification key, the
// stand-alone quotient operator) reads bj::GateShape records made here, and every refusal about a gate descriptor or about the
// layout of the specialized columns is worded here.  Plain C++17 over include/boojum_hip.h: a host program can use it.
#pragma once
#include "../../include/boojum_hip.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

namespace bj {

// One gate as its evaluators take it.  General-purpose gates read variable columns r * var_stride + i, constant columns
// path_len + r * const_stride + i and witness columns r * wit_stride + i of repetition r; gates over specialized columns have no
// selector path and start at (first_col, first_const).  Its alpha powers are [first_term, first_term + terms()) of its category.
struct GateShape {
    int kind = 0;
    unsigned path_len = 0;
    unsigned char path[8] = {};   // 1: constant column b, 0: 1 - constant column b
    unsigned reps = 0, var_stride = 0, const_stride = 0, wit_stride = 0, num_terms = 0;
    unsigned first_col = 0, first_const = 0;
    unsigned first_term = 0;
    unsigned terms() const { return reps * num_terms; }
};

// What a hand-written kind reads, relative to its repetition (constants: after the selector path).  const_per_rep: every
// repetition has its own constants, const_stride apart; otherwise the repetitions share them.  fixed_terms: the terms per
// repetition its descriptor must declare (0: any).  single_rep: one repetition over the first var_extent columns.
struct GateKindExtent {
    unsigned var_extent, const_extent;
    bool const_per_rep;
    unsigned fixed_terms;
    bool single_rep;
};
inline GateKindExtent gate_kind_extent(int kind) {
    switch (kind) {
        case BJ_GATE_CONSTANT_ALLOCATOR: return {1, 1, true, 1, false};
        case BJ_GATE_FMA_NO_CONSTANT: return {4, 2, false, 1, false};
        case BJ_GATE_REDUCTION4: return {5, 4, false, 1, false};
        case BJ_GATE_POSEIDON2_FLATTENED:
        case BJ_GATE_POSEIDON_FLATTENED: return {130, 0, true, 118, true};
        default: return {0, 0, true, 0, false};   // BJ_GATE_NOP reads nothing; an op list's extents are gate_program_extent's
    }
}

// highest variable / constant / witness column index (relative to the repetition) an op list reads, + 1; 0 if it reads none
inline void gate_program_extent(const bj_gate_program *p, unsigned *var_extent, unsigned *const_extent, unsigned *wit_extent = nullptr) {
    unsigned v = 0, c = 0, w = 0;
    auto see = [&](const bj_gate_index &ix) {
        if (ix.kind == BJ_IDX_VARIABLE_POLY && ix.index + 1 > v) v = ix.index + 1;
        if (ix.kind == BJ_IDX_CONSTANT_POLY && ix.index + 1 > c) c = ix.index + 1;
        if (ix.kind == BJ_IDX_WITNESS_POLY && ix.index + 1 > w) w = ix.index + 1;
    };
    for (uint32_t i = 0; p && p->relations && i < p->num_relations; i++) {
        const bj_gate_relation &R = p->relations[i];
        see(R.a);
        if (R.op == BJ_OP_ADD || R.op == BJ_OP_SUB || R.op == BJ_OP_MUL) see(R.b);
    }
    for (uint32_t t = 0; p && p->writes && t < p->num_writes; t++) see(p->writes[t]);
    *var_extent = v;
    *const_extent = c;
    if (wit_extent) *wit_extent = w;
}

struct GateList {
    std::vector<GateShape> general, spec;          // evaluator order / declaration order
    unsigned n_general_terms = 0, n_spec_terms = 0;
    void push_general(GateShape s) {
        s.first_term = n_general_terms;
        n_general_terms += s.terms();
        general.push_back(s);
    }
    void push_spec(GateShape s) {
        s.first_term = n_spec_terms;
        n_spec_terms += s.terms();
        spec.push_back(s);
    }
};

inline int gate_refusal(std::string *err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
    return code;
}

inline GateShape gate_shape_of(const bj_gate_desc &G) {
    GateShape s;
    s.kind = G.kind;
    s.path_len = G.path_len;
    for (unsigned b = 0; b < G.path_len && b < 8; b++) s.path[b] = G.path[b] ? 1 : 0;
    s.reps = G.num_repetitions; s.var_stride = G.var_stride; s.const_stride = G.const_stride; s.wit_stride = G.wit_stride;
    s.num_terms = G.num_terms;
    return s;
}

// the columns a gate over general-purpose columns may read
struct GateColumns {
    unsigned variables, constants, witnesses;
};

// Gate g over general-purpose columns: BJ_OK and its shape (first_term is GateList::push_general's), or the refusal in *err.
// Every column index the evaluator will form must exist: (reps - 1) * stride + the widest operand, after the selector path.
// past_the_columns: what an entry point whose caller hands over the columns themselves says instead of the column numbers.
inline int resolve_gate(const bj_gate_desc &G, unsigned g, const GateColumns &cols, GateShape *out, std::string *err,
                        const char *past_the_columns = nullptr) {
    GateKindExtent e = gate_kind_extent(G.kind);
    if (G.kind < 1 || G.kind > BJ_GATE_POSEIDON_FLATTENED || G.path_len > 6 || (G.kind == BJ_GATE_PROGRAM && !G.program) ||
        (e.single_rep && (G.num_repetitions != 1 || cols.variables < e.var_extent)) || (e.fixed_terms && G.num_terms != e.fixed_terms))
        return gate_refusal(err, BJ_ERR_INVALID_ARG, "bad gate descriptor %u", g);
    unsigned wit_extent = 0;
    if (G.kind == BJ_GATE_PROGRAM) gate_program_extent(G.program, &e.var_extent, &e.const_extent, &wit_extent);
    const size_t last = G.num_repetitions ? G.num_repetitions - 1 : 0;
    if (wit_extent && last * G.wit_stride + wit_extent > cols.witnesses)
        return gate_refusal(err, BJ_ERR_INVALID_ARG, "gate %u reads witness column %zu of %u", g,
                            (size_t)(G.num_repetitions - 1) * G.wit_stride + wit_extent, cols.witnesses);
    const size_t var_end = e.var_extent ? last * G.var_stride + e.var_extent : 0;
    const size_t const_end = G.path_len + (e.const_extent ? (e.const_per_rep ? last * G.const_stride : 0) + e.const_extent : 0);
    if (G.kind != BJ_GATE_NOP && (G.num_repetitions == 0 || var_end > cols.variables || const_end > cols.constants)) {
        if (past_the_columns) return gate_refusal(err, BJ_ERR_INVALID_ARG, "gate %u %s", g, past_the_columns);
        return gate_refusal(err, BJ_ERR_INVALID_ARG, "gate %u reads variable column %zu / constant column %zu of %u / %u "
                            "(repetitions x stride + operand index, after a selector path of %u)", g, var_end, const_end,
                            cols.variables, cols.constants, G.path_len);
    }
    if (G.path_len > cols.constants) return gate_refusal(err, BJ_ERR_INVALID_ARG, "gate %u: selector path longer than the constant columns", g);
    if (G.kind == BJ_GATE_PROGRAM && G.program->num_writes != G.num_terms)
        return gate_refusal(err, BJ_ERR_INVALID_ARG, "gate %u: program writes %u terms, descriptor says %u", g, G.program->num_writes,
                            G.num_terms);
    *out = gate_shape_of(G);
    return BJ_OK;
}

// A check of an op list that is not plain C++ over the C header (canonicalisation), run where a program has passed every other
// check on its gate.  It words its own refusal: *err stays empty and its status is returned as it is.
using GateProgramCheck = std::function<int(const bj_gate_program *)>;

// Every gate of the circuit and the layout of the specialized columns: BJ_OK and the resolved list, or the first refusal (the
// message in *err, to go behind the caller's name).  lookup_cps: variable columns of one lookup sub-argument.
inline int resolve_gates(const bj_circuit &c, unsigned lookup_cps, GateList *out, std::string *err,
                         const GateProgramCheck &check_program = nullptr) {
    *out = GateList{};
    err->clear();
    if (c.num_gates > 16)
        return gate_refusal(err, BJ_ERR_UNSUPPORTED, "%u gate types over general-purpose columns (at most 16)", c.num_gates);
    const GateColumns cols{c.num_gp_vars, c.num_constant_cols, c.num_witness_cols};
    for (unsigned g = 0; g < c.num_gates; g++) {
        GateShape s;
        if (int rc = resolve_gate(c.gates[g], g, cols, &s, err)) return rc;
        if (s.kind == BJ_GATE_PROGRAM && check_program)
            if (int rc = check_program(c.gates[g].program)) return rc;
        out->push_general(s);
    }
    // gates over specialized columns (evaluator_data.rs:124-240, prover.rs:635-800): their variable columns follow the lookup ones
    // in declaration order; their constant columns follow the general-purpose gates' ones and the table-id column (which is the
    // first "special purpose" constant: setup.rs:963-1010), num_repetitions * const_stride columns each — every repetition its
    // own principal_width.num_constants columns (share_constants = false, per_repetition_offset.constants_offset = that width)
    // (64-bit sums: the sizes are the caller's, a wrapped 32-bit total must not pass the range checks)
    const bool tid_const = c.lookup_reps && c.table_id_col != BJ_TABLE_ID_AS_VARIABLE;
    uint64_t col = (uint64_t)c.num_gp_vars + (uint64_t)lookup_cps * c.lookup_reps;
    uint64_t spec_consts = 0;
    for (unsigned g = 0; c.specialized_gates && g < c.num_specialized_gates; g++) {
        const uint64_t per_gate = (uint64_t)c.specialized_gates[g].num_repetitions * c.specialized_gates[g].const_stride;
        if (per_gate > c.num_constant_cols) { spec_consts = (uint64_t)c.num_constant_cols + 1; break; }
        spec_consts += per_gate;
    }
    if (spec_consts > c.num_constant_cols || (tid_const && (uint64_t)c.table_id_col + 1 + spec_consts != c.num_constant_cols))
        return gate_refusal(err, BJ_ERR_INVALID_ARG, "%u constant columns declared; the specialized gates' %llu must be the "
                            "last ones, right behind the table-id column", c.num_constant_cols, (unsigned long long)spec_consts);
    unsigned ccol = c.num_constant_cols - (unsigned)spec_consts;
    for (unsigned g = 0; g < c.num_specialized_gates; g++) {
        const bj_gate_desc *G = c.specialized_gates ? &c.specialized_gates[g] : nullptr;
        bool ok = G && G->kind == BJ_GATE_PROGRAM && G->program && G->path_len == 0 && G->num_repetitions && G->var_stride &&
                  G->program->num_writes == G->num_terms;
        if (ok) {
            // a repetition reads its own var_stride variable columns and its own const_stride constant columns, no witness column.
            // Constants SHARED by the repetitions (share_constants = true with constants) are refused: the reference itself hands
            // such an evaluator an empty constant range (per_repetition_offset.constants_offset = 0, prover.rs:748-772)
            unsigned ve = 0, ce = 0, we = 0;
            gate_program_extent(G->program, &ve, &ce, &we);
            ok = ve <= G->var_stride && we == 0 && ce <= G->const_stride;
        }
        if (!ok)
            return gate_refusal(err, BJ_ERR_UNSUPPORTED, "specialized gate %u must be an op list without a selector path "
                                "whose repetitions each read their own var_stride variable and const_stride constant columns "
                                "(share_constants = false) and no witness column", g);
        if (check_program)
            if (int rc = check_program(G->program)) return rc;
        if (col + (uint64_t)G->num_repetitions * G->var_stride > c.num_vars)
            return gate_refusal(err, BJ_ERR_INVALID_ARG, "specialized gate %u runs past the %u declared variable columns", g, c.num_vars);
        GateShape s = gate_shape_of(*G);
        s.first_col = (unsigned)col;
        s.first_const = ccol;
        out->push_spec(s);
        col += (uint64_t)s.reps * s.var_stride;
        ccol += s.reps * s.const_stride;
    }
    if (col != c.num_vars)
        return gate_refusal(err, BJ_ERR_INVALID_ARG, "%u variable columns declared, geometry + lookups + "
                            "specialized gates make %llu", c.num_vars, (unsigned long long)col);
    return BJ_OK;
}

}  // namespace bj
