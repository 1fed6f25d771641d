// Internal: what the launchers of the term kernels (rounds 2 and 3: copy-permutation, lookup, every gate evaluator) are given,
// as values instead of positional pointer lists.  A d_ field is a device pointer, an h_ field a host pointer; F_p^2 challenges are
// two words, alpha powers [count][2].
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bj {
typedef uint64_t u64;

// a column-major batch on the device: column c starts at p + c * stride
struct Cols {
    const u64 *p;
    size_t stride;
    Cols at(size_t c) const { return {p + c * stride, stride}; }   // the batch that starts at column c
};

// the columns a gate evaluator reads; the witness (non-copiable) columns lie at vars.stride, wits is null if there are none
struct GateCols {
    Cols vars, consts;
    const u64 *wits;
};

// Where terms go: out += (or =, as the launcher says) sum alpha * term at `points` points.  d_alphas is the first power of the
// gate's CATEGORY (general-purpose, specialized, lookup, copy-permutation chunks): a launcher of one gate G adds 2 * G.first_term
// itself, through powers().  Null stays null: stand-alone term mode of the op-list evaluator, which has no weights and no accumulators.
struct TermSink {
    const u64 *d_alphas;
    size_t points;
    u64 *out0, *out1;
    const u64 *powers(size_t first_term) const { return d_alphas ? d_alphas + 2 * first_term : nullptr; }
};

// the copy-permutation argument over V columns in chunks of `chunk`
struct CopyPermArg {
    Cols vars, sigmas;
    const u64 *d_non_res;      // [V]
    unsigned V, chunk, log_n;
    const u64 *d_tw;           // forward twiddle table of the domain the columns are on
    const u64 *h_beta, *h_gamma;
    bool small_non_residues;   // every non-residue is below 2^32 (canonical)
};

// the lookup argument: reps sub-arguments of width w over the table columns
struct LookupArg {
    Cols lvars, tables;
    const u64 *d_table_id;     // null: the id is the last of the w + 1 variable columns of every sub-argument
    const u64 *d_mult;
    unsigned reps, w;
    const u64 *h_beta, *h_gamma;
};
}  // namespace bj
