// Internal: from a bj::GateShape (gate_list.h) to what a gate kernel takes — the argument structs of the hand-written kernels of
// quotient.hip and the host functions that fill them and the op-list evaluators' ProgArgs.  Host code only; the one place where a
// shape's path, repetitions and strides are unpacked.
#pragma once
#include "gate_program.h"

namespace bj {

struct GateDev {
    int kind, path_len, reps, var_stride, const_stride, num_terms;
    int path[6];
};
// the kinds the two kernels below evaluate themselves (bj_gate_kind); every kind from BJ_GATE_PROGRAM on has a kernel of its own
constexpr int K_ALLOC = BJ_GATE_CONSTANT_ALLOCATOR, K_FMA = BJ_GATE_FMA_NO_CONSTANT, K_RED4 = BJ_GATE_REDUCTION4;
constexpr int BJ_MAX_GATES = 16;   // evaluators over general-purpose columns per circuit (the golden proof's circuit has 11)
struct GateSet {
    GateDev g[BJ_MAX_GATES];
    int n_gates;
};
constexpr int GW_WINDOW = 20;
struct GateWindows {
    int present[BJ_GATE_NOP];   // by kind (K_ALLOC, K_FMA, K_RED4)
    int path_len[BJ_GATE_NOP], path[BJ_GATE_NOP][6];
    int reps[BJ_GATE_NOP], const_stride[BJ_GATE_NOP], aoff[BJ_GATE_NOP];
    int n_windows, n_vars;
};

// the first n (at most BJ_MAX_GATES) gates of a list for quotient_gates_kernel, which walks the alpha powers itself, in list order
inline GateSet gate_set(const GateShape *gates, unsigned n) {
    GateSet gs;
    gs.n_gates = (int)n;
    for (unsigned g = 0; g < n && g < (unsigned)BJ_MAX_GATES; g++) {
        const GateShape &G = gates[g];
        gs.g[g] = GateDev{G.kind, (int)G.path_len, (int)G.reps, (int)G.var_stride, (int)G.const_stride, (int)G.num_terms,
                          {G.path[0], G.path[1], G.path[2], G.path[3], G.path[4], G.path[5]}};
    }
    return gs;
}

// The list for quotient_gates_windowed_kernel; false when that kernel cannot take it: it wants the hand-written kinds at most once
// each, with their principal widths, one term per repetition, shared constants (but the allocator's) and a path of at most 6.
// Gates without terms and the kinds with kernels of their own are passed over; a list with no hand-written gate is refused too.
inline bool gate_windows(const GateShape *gates, unsigned n, GateWindows *out) {
    GateWindows gw{};
    int span = 0, n_hand = 0;
    for (unsigned g = 0; g < n; g++) {
        const GateShape &G = gates[g];
        if (G.num_terms == 0 || G.kind >= BJ_GATE_PROGRAM) continue;
        const int width = (int)gate_kind_extent(G.kind).var_extent;
        if (G.kind < K_ALLOC || G.kind >= BJ_GATE_NOP || gw.present[G.kind] || (int)G.var_stride != width || G.num_terms != 1 || G.path_len > 6 ||
            (G.kind != K_ALLOC && G.const_stride != 0))
            return false;
        gw.present[G.kind] = 1;
        gw.path_len[G.kind] = (int)G.path_len;
        for (int b = 0; b < 6; b++) gw.path[G.kind][b] = G.path[b];
        gw.reps[G.kind] = (int)G.reps;
        gw.const_stride[G.kind] = (int)G.const_stride;
        gw.aoff[G.kind] = (int)G.first_term;
        if ((int)G.reps * width > span) span = (int)G.reps * width;
        n_hand++;
    }
    gw.n_windows = (span + GW_WINDOW - 1) / GW_WINDOW;
    gw.n_vars = span;
    *out = gw;
    return n_hand > 0;
}

// bit b: the selector takes constant column b (otherwise 1 - it), as the Poseidon gate kernels take a path
inline unsigned path_bits(const GateShape &G) {
    unsigned bits = 0;
    for (unsigned b = 0; b < G.path_len; b++) bits |= (G.path[b] ? 1u : 0u) << b;
    return bits;
}

// An op-list gate for the interpreter, a generated or a run-time compiled kernel; d_terms: stand-alone term mode, or null.  Only a
// program that reads witness columns is given them: the fused launch of the generated bodies (gate_aot.hip) refuses an entry that
// carries any, and its gates sweep a circuit's columns whether or not the circuit has witness columns.
inline gpdev::ProgArgs prog_args(const DevProgram &P, const GateShape &G, const GateCols &c, const TermSink &o, gl::u64 *d_terms) {
    gpdev::ProgArgs a{};
    a.vars = c.vars.p; a.var_stride = c.vars.stride; a.consts = c.consts.p; a.const_stride = c.consts.stride;
    if (P.reads_witness) { a.wits = c.wits; a.rep_wit_stride = G.wit_stride; }
    a.rel = P.d_rel; a.values = P.d_values; a.n_rel = P.n_rel; a.n_writes = P.n_writes;
    a.path_len = G.path_len;
    for (unsigned b = 0; b < 8; b++) a.path[b] = b < G.path_len ? G.path[b] : 0;
    a.reps = G.reps; a.rep_var_stride = G.var_stride; a.rep_const_stride = G.const_stride;
    a.alphas = o.powers(G.first_term);
    a.Q = o.points; a.out0 = o.out0; a.out1 = o.out1; a.terms = d_terms;
    return a;
}
}  // namespace bj
