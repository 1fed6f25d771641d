// Internal: the setup object behind the opaque `bj_setup` of include/boojum_hip.h, shared by setup.hip (which creates it),
// prover.hip (which proves with it), check_satisfied.hip (which only reads the replicated natural-order columns and the gate list)
// and verifier.hip (bj_vk_from_setup copies the shape, the gate list and the packed op lists).  The circuit's shape and every
// column position are proof_layout.h's: that header is the definition of what an oracle holds and of a proof's word order.
#pragma once
#include "ctx.h"
#include "fri_types.h"
#include "gate_program.h"
#include "oracle_value.h"
#include "proof_layout.h"

#include <vector>

struct bj_setup : bj::CircuitShape {   // proof_layout.h: bj::circuit_shape fills the base
    int device = 0;
    bj::ProofLayout layout;        // of this shape: column positions, leaf widths, opening order
    bj::GateList gates;            // as bj::resolve_gates (gate_list.h) made it from the circuit's description
    std::vector<bj::DevProgram> programs, spec_programs;   // beside gates.general / gates.spec; empty (block == nullptr) unless kind == BJ_GATE_PROGRAM
    std::vector<gl::u64> non_residues;
    bool small_non_residues = false;   // every k_c < 2^32 (canonical): quotient_copy_perm multiplies by them as 32-bit integers
    std::vector<unsigned> pub_cols, pub_rows;
    // proof config
    unsigned fri_lde = 0, security = 0, pow_bits = 0, transcript = BJ_TRANSCRIPT_POSEIDON2, hasher = BJ_HASHER_POSEIDON2;
    unsigned pow_runner = BJ_POW_BLAKE2S256;   // the POW type parameter of prove_cpu_basic (pow.rs:6-31)
    unsigned L = 0, log_L = 0, log_q = 0;
    // shard of the LDE domain held by this GPU: cosets [c0, c0 + cl), i.e. flat indices [c0*n, (c0+cl)*n)
    bj::Shard sh;
    unsigned c0 = 0, cl = 0;
    size_t Ls = 0;                 // column stride of every LDE array = cl * n
    size_t Nl = 0;                 // Merkle leaves held here (n * fri_lde / world)
    size_t cap_l = 0;              // cap nodes of the local subtree (cap_size / world)
    gl::u64 *d_nat = nullptr;          // [setup width][n] natural-order values (replicated)
    gl::u64 *d_mono = nullptr;         // [setup width][n] monomial forms (replicated; the DEEP numerator is combined on them)
    bool tiled = false;            // monomials (these and every proof's) in the tiled layout of ntt_r16.hip: 2^22-row traces
    gl::u64 *d_lde = nullptr;          // [setup width][cl][n]; null once a lean setup stands
    bool lean = false;             // BJ_SETUP_LEAN as it stood when the setup was created: the LDE is not kept, a proof rebuilds the quotient's
                                   // cosets from d_mono one at a time and evaluates the queried leaves (prover.hip); never set on a shard
    gl::u64 *d_tree = nullptr;         // local subtree
    gl::u64 *d_non_res = nullptr;
    gl::u64 *d_inv_xm1 = nullptr;      // 1 / (x - 1) on the points this GPU evaluates the quotient on (a property of the domain)
    uint32_t *d_placement = nullptr;   // bj_setup_create_from_placement: variable index per cell [V][n], PLACEMENT_NONE = placeholder
    uint32_t *d_wit_placement = nullptr;   // bj_setup_set_witness_placement: the same for the non-copiable witness columns [Wc][n]
    // host copy of the placement entries at the public input locations (one per location, PLACEMENT_NONE where the placement that
    // covers the column is not held): the public values of a proof from values are all_values[entry], read on the host
    std::vector<uint32_t> pub_place;
    std::vector<gl::u64> cap;

    // The setup's committed oracle as a value (oracle_value.h).  A lean setup has no evaluations of its own: a proof points the value at
    // a [width][n] coset buffer of its workspace
    bj::Oracle oracle() const {
        bj::Oracle o = bj::oracle_of(layout.widths[bj::ORACLE_SETUP], (size_t)1 << log_n, Ls, !lean);
        o.mono = d_mono, o.evals = d_lde, o.tree = d_tree;
        return o;
    }
};


namespace bj {
// the tree kernels of the calls in its scope follow the proof config, then the context's own setting returns
struct HasherGuard {
    bj_ctx *c;
    int saved;
    ~HasherGuard() { c->hasher = saved; }
};

// quotient.hip: every gate evaluator of the setup's circuit on caller-given columns; general OVERWRITES its sink with the gates over
// general-purpose columns, spec ADDS the gates over specialized columns to its own; a null sink skips that part
void launch_circuit_gates(bj_ctx *ctx, const bj_setup *S, Cols vars, Cols consts, const TermSink *general, const TermSink *spec, hipStream_t st);
}  // namespace bj
