// Internal: the host side of the opening stage's kernel arguments.  Every kernel of openings.hip reads BASE columns with F_p^2
// coefficients; the callers speak of SOURCES, each a base column or an F_p^2 polynomial stored as the column pair (c0, c1).
// The rule that turns one into the other is written here once, with its inverse:
//   (f0 + f1 u) * (ch0 + ch1 u) = f0 * (ch0 + ch1 u) + f1 * (7 ch1 + ch0 u)           (u^2 = 7)
// so an F_p^2 source with challenge ch adds its column c1 with the coefficient (7 ch1, ch0), and a set's constant is
// C = sum_k ch_k * v_k.  Plain C++, free of HIP like callee_words.h: a host program checks it (tests/opening_args_check.cpp).
#pragma once
#include "callee_words.h"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bj {
struct OpenSrc { const uint64_t *c0, *c1; };   // a base-field column (c1 == nullptr) or the two columns of an F_p^2 polynomial

// sources given as two host arrays, as the C ABI has them: a null c1 array or a null entry in it is a base-field source
inline std::vector<OpenSrc> open_srcs(const uint64_t *const *c0, const uint64_t *const *c1, size_t n_src) {
    std::vector<OpenSrc> s(n_src);
    for (size_t k = 0; k < n_src; k++) s[k] = OpenSrc{c0[k], c1 ? c1[k] : nullptr};
    return s;
}

namespace open_fp {   // Goldilocks on the host, any u64 representative in, canonical out
constexpr uint64_t P = 0xFFFFFFFF00000001ULL;
inline uint64_t residue(uint64_t a) { return a >= P ? a - P : a; }
inline uint64_t add(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % P); }
inline uint64_t mul(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % P); }
}  // namespace open_fp

inline void push_columns(std::vector<const uint64_t *> &ptrs, const OpenSrc &s) {   // the base columns of one source
    ptrs.push_back(s.c0);
    if (s.c1) ptrs.push_back(s.c1);
}

// One opening set of a ColumnList: its columns [first_col, first_col + n_cols), its constant C and its point, canonical
struct ColumnSet {
    size_t first_col;
    unsigned n_cols;
    uint64_t C[2], at[2];
};

// Opening sets flattened into one list of base columns with F_p^2 coefficients; what goes to the device is one block,
// [pointers][coefficients], of words() words.
struct ColumnList {
    std::vector<const uint64_t *> ptrs;
    std::vector<uint64_t> coefs;       // [n_cols][2], canonical
    std::vector<ColumnSet> sets;
    bool ok = true;                    // false once a source without a column was met: the list is unusable
    size_t bad_src = 0, bad_set = 0;   // that source and its set

    // Appends the set of n_src sources with challenges [n_src][2], values [n_src][2] (null: all zero, C = 0) and the point
    // at2 (null: zero).  False, and nothing more is taken, if a source has no c0.
    bool add_set(const OpenSrc *srcs, size_t n_src, const uint64_t *challenges, const uint64_t *values, const uint64_t *at2) {
        using namespace open_fp;
        if (!ok) return false;
        ColumnSet S{ptrs.size(), 0, {0, 0}, {at2 ? residue(at2[0]) : 0, at2 ? residue(at2[1]) : 0}};
        for (size_t k = 0; k < n_src; k++) {
            if (!srcs[k].c0) {
                ok = false, bad_src = k, bad_set = sets.size();
                return false;
            }
            const uint64_t ch0 = residue(challenges[2 * k]), ch1 = residue(challenges[2 * k + 1]);
            if (values) {   // C += ch * v
                const uint64_t v0 = values[2 * k], v1 = values[2 * k + 1];
                S.C[0] = add(S.C[0], add(mul(ch0, v0), mul(7, mul(ch1, v1))));
                S.C[1] = add(S.C[1], add(mul(ch0, v1), mul(ch1, v0)));
            }
            push_columns(ptrs, srcs[k]);
            coefs.insert(coefs.end(), {ch0, ch1});
            if (srcs[k].c1) coefs.insert(coefs.end(), {mul(7, ch1), ch0});
        }
        S.n_cols = (unsigned)(ptrs.size() - S.first_col);
        sets.push_back(S);
        return true;
    }
    size_t n_cols() const { return ptrs.size(); }
    size_t ptr_offset() const { return 0; }              // of the pointers and of the coefficients, in words of the block
    size_t coef_offset() const { return ptrs.size(); }
    size_t words() const { return coef_offset() + coefs.size(); }   // = column_list_arg_words(n_cols()), what the workspace plan allows
};

// The base columns of a list of sources in the order add_set flattens them: what is evaluated to open them
inline std::vector<const uint64_t *> open_columns(const OpenSrc *srcs, size_t n_src) {
    std::vector<const uint64_t *> ptrs;
    for (size_t k = 0; k < n_src; k++) push_columns(ptrs, srcs[k]);
    return ptrs;
}
// The inverse of the flattening: F_p^2 values flat [n_cols][2] of those columns -> one value per source, out [n_src][2]:
// E(c0) + u * E(c1) = (a0 + 7 b1, a1 + b0)
inline void recombine_values(const OpenSrc *srcs, size_t n_src, const uint64_t *flat, uint64_t *out) {
    using namespace open_fp;
    for (size_t k = 0, c = 0; k < n_src; k++, c++) {
        out[2 * k] = residue(flat[2 * c]);
        out[2 * k + 1] = residue(flat[2 * c + 1]);
        if (srcs[k].c1) {
            c++;
            out[2 * k] = add(out[2 * k], mul(7, flat[2 * c + 1]));
            out[2 * k + 1] = add(out[2 * k + 1], flat[2 * c]);
        }
    }
}
}  // namespace bj
