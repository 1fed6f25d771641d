// Internal: device-side form of a bj_gate_program (seam S3), shared by gate_program.hip, setup.hip and prover.hip.
#pragma once
#include "ctx.h"
#include "gate_body_rt.h"
#include "gate_canon.h"
#include "gate_list.h"

#include <vector>

// slots of the interpreter's private (scratch-memory) variant; the canonical form of gate_canon.h needs far fewer for every
// evaluator of the reference (13 for a 12 x 12 matrix gate, ~40 for the Poseidon2 flattened capture); a program whose
// schedule needs more than BJ_GATE_PROGRAM_MAX_SLOTS live values at once is refused
#define BJ_GATE_PROGRAM_MAX_TEMPORARIES 160
#define BJ_GATE_PROGRAM_MAX_SLOTS 1024

namespace bj {
struct JitKernel;             // gate_jit.hip: a kernel compiled at run time from the canonical program
struct DevProgram {
    void *block = nullptr;    // one allocation: values | relations
    gl::u64 *d_values = nullptr;
    DevRelation *d_rel = nullptr;
    unsigned n_rel = 0, n_writes = 0, n_tmp = 0;   // n_rel counts the OP_WRITE pseudo relations; n_tmp: slots
    bool reads_witness = false;   // the program has BJ_IDX_WITNESS_POLY operands
    unsigned var_extent = 0, const_extent = 0, wit_extent = 0;
    uint64_t fp[2] = {0, 0};      // structural fingerprint (gate_canon.h): selects a generated kernel when one exists
    const JitKernel *jit = nullptr;   // compiled at upload when no generated kernel exists (owned by the process-wide cache)
    std::vector<DevRelation> h_rel;   // host copy of what d_rel / d_values hold: a verification key takes its op lists from here
    std::vector<gl::u64> h_values;
    int upload(bj_ctx *ctx, const bj_gate_program *p);   // canonicalises, packs and copies the program
    void release();
};
// the canonical program in the interpreter's packed form (operands kind << 28 | slot or index, OP_WRITE pseudo relations)
void pack_program(const canon::Program &C, std::vector<DevRelation> *rel, std::vector<gl::u64> *values);
// The launchers below take the columns and the destination as term_io.h's descriptors; out.d_alphas is the first power of the
// gates' category, as everywhere (TermSink).
// gate G with op list P.  Quotient mode (out.d_alphas != nullptr): out += selector * sum alpha * term; stand-alone mode
// (d_terms != nullptr): raw terms [reps * n_writes][out.points]
void launch_gate_program(const DevProgram &P, const GateShape &G, const GateCols &cols, const TermSink &out, gl::u64 *d_terms, hipStream_t s);
// the op-list gates of a gate list (quotient mode); programs[g] belongs to gates[g]
void launch_gate_programs(const GateShape *gates, const DevProgram *programs, unsigned n, const GateCols &cols, const TermSink &out, hipStream_t s);
// quotient.hip: every evaluator of a list of gates over general-purpose columns; probe_bytes: algorithmic bytes of the
// hand-written launch, for the kernel probe of a proof
void launch_general_gates(bj_ctx *ctx, const GateShape *gates, const DevProgram *programs, unsigned n_gates, const GateCols &cols,
                          const TermSink &out, hipStream_t st, double probe_bytes);
}  // namespace bj
