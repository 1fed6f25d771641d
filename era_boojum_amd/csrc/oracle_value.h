// A committed oracle of a proof, as a value: the witness, stage-2, quotient and setup oracles in proof_layout.h's ORACLE_* order.
// An oracle is its monomials, its tree, and its evaluations, which it either keeps (resident: every coset this rank holds) or
// rebuilds from the monomials one coset at a time into a [width][n] buffer (lean: bj_setup::lean for the setup's, BJ_PROOF_LEAN
// for the witness and stage 2; the quotient is always resident, on the FRI domain).  What follows from that bit is answered here
// and nowhere else: where the columns of a coset are, where an opened polynomial is, whether an opening set can be read on the
// FRI domain, how a queried leaf's words are made.  The prover asks the values, the workspace plan the same functions.
// Plain C++17, no HIP: a host program can use it (tests/oracle_check.cpp).
#pragma once
#include "opening_args.h"
#include "proof_layout.h"
#include "term_io.h"

namespace bj {

struct Oracle {
    unsigned width = 0;
    size_t n = 0;                    // points of a coset; monomial columns lie n apart
    // column c of the monomials starts at mono + (c % mono_parts) * mono_part_gap + (c / mono_parts) * n.  One part: [width][n].
    // The quotient's are T's chunk layout, two parts (the F_p^2 components) Q apart, chunk j of each at j * n: column 2 j + e
    const uint64_t *mono = nullptr;
    unsigned mono_parts = 1;
    size_t mono_part_gap = 0;
    uint64_t *evals = nullptr;       // resident: [width][stride], the cosets this rank holds; lean: [width][n], ONE coset
    size_t stride = 0;               // of evals: the points this rank holds of a column, or n
    uint64_t *tree = nullptr;
    bool resident = true;

    // The oracle's columns at coset c of this rank.  Lean: the coset buffer, which holds coset c only once it was rebuilt for c
    Cols cols_at(size_t c) const { return resident ? Cols{evals + c * n, stride} : Cols{evals, stride}; }
    const uint64_t *mono_col(unsigned c) const { return mono + (c % mono_parts) * mono_part_gap + (size_t)(c / mono_parts) * n; }
    // An opened polynomial on the evaluations, from this rank's first coset on (lean: the coset the buffer holds), and on the monomials
    OpenSrc eval_src(const Opened &o) const { return {evals + o.col0 * stride, o.col1 == NO_COLUMN ? nullptr : evals + o.col1 * stride}; }
    OpenSrc mono_src(const Opened &o) const { return {mono_col(o.col0), o.col1 == NO_COLUMN ? nullptr : mono_col(o.col1)}; }
    // A queried leaf's words: gathered from the evaluations, or (false) the monomials evaluated at the leaf's point
    bool leaf_from_evals() const { return resident; }
    size_t eval_words() const { return (size_t)width * stride; }
};

// An oracle of `width` columns on cosets of n points, of which this rank holds `held` points per column when it is resident.
// The pointers are the owner's to set.
inline Oracle oracle_of(unsigned width, size_t n, size_t held, bool resident) {
    Oracle o;
    o.width = width, o.n = n, o.resident = resident, o.stride = resident ? held : n;
    return o;
}

// Sets of oracles as bit masks, bit ORACLE_*
inline unsigned oracle_mask(const std::vector<Opened> &polys) {
    unsigned m = 0;
    for (const Opened &o : polys) m |= 1u << o.oracle;
    return m;
}
inline unsigned base_columns(const std::vector<Opened> &polys) {   // an F_p^2 polynomial counts two
    unsigned c = 0;
    for (const Opened &o : polys) c += o.col1 == NO_COLUMN ? 1 : 2;
    return c;
}
inline unsigned resident_mask(bool lean_setup, bool lean_proof) {
    return 1u << ORACLE_QUOTIENT | (lean_setup ? 0u : 1u << ORACLE_SETUP) | (lean_proof ? 0u : 1u << ORACLE_WITNESS | 1u << ORACLE_STAGE2);
}
inline unsigned resident_mask(const Oracle (&oracles)[4]) {
    unsigned m = 0;
    for (unsigned k = 0; k < 4; k++)
        if (oracles[k].resident) m |= 1u << k;
    return m;
}
// DEEP can stream an opening set over the FRI domain iff every polynomial of it belongs to an oracle whose evaluations are there;
// any other set is combined on its monomials and extended, whatever its size
inline bool can_stream(unsigned set_oracles, unsigned resident) { return !(set_oracles & ~resident); }

}  // namespace bj
