// Internal: the host arithmetic of bj_list_unsatisfied (list_unsatisfied.hip) — how many trace rows one term-evaluation chunk
// holds, how many entry slots the device block gets, and how a capacity falls across the four kinds once their totals are known.
// Plain C++ over <stdint.h>, no HIP call: tests/list_plan_check.cpp includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bj {

constexpr unsigned LIST_BLOCK = 256;            // threads per block of the listing's kernels; chunk rows are a multiple of it
constexpr uint64_t LIST_CHUNK_MAX = 16384;      // most rows of one chunk: (columns + 2 * terms) * 16384 words of scratch

inline uint64_t list_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
inline uint64_t list_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Rows per chunk of the per-term evaluation: the capacity padded to the block (every failing row yields at least one entry, so
// the rows that can reach the output fit the first chunk), between `lo` and `hi`.  hi keeps the scratch bounded, lo keeps the
// number of count-only chunks of a long flagged list at 64 or fewer per 2^20 rows.  n: trace rows, a power of two >= LIST_BLOCK
// or smaller (then the one chunk is padded to a block).
inline uint64_t list_chunk_rows(uint64_t capacity, uint64_t n) {
    const uint64_t n_pad = (list_max(n, 1) + LIST_BLOCK - 1) / LIST_BLOCK * LIST_BLOCK;
    const uint64_t hi = list_min(n_pad, LIST_CHUNK_MAX);
    const uint64_t lo = list_min(hi, list_max(LIST_BLOCK, n / 64));
    const uint64_t cap_pad = capacity > hi ? hi : (list_max(capacity, 1) + LIST_BLOCK - 1) / LIST_BLOCK * LIST_BLOCK;
    return list_min(hi, list_max(lo, cap_pad));
}
inline uint64_t list_chunks(uint64_t flagged_rows, uint64_t chunk_rows) { return (flagged_rows + chunk_rows - 1) / chunk_rows; }

// saturating a * b + c (a trace cannot have more entries than this, and a capacity above it needs no more slots)
inline uint64_t list_mul_add_sat(uint64_t a, uint64_t b, uint64_t c) {
    if (a && b > (UINT64_MAX - c) / a) return UINT64_MAX;
    return a * b + c;
}
// Entry slots of the device block: the capacity, or the most entries a trace of n rows can have if that is less — per row the
// terms of its one selected general-purpose gate (at most max_general_terms) and every specialized term, one per (row,
// sub-argument), one per table row.
inline uint64_t list_entry_slots(uint64_t capacity, uint64_t n, uint64_t max_general_terms, uint64_t spec_terms, uint64_t lookup_reps) {
    const uint64_t per_row = max_general_terms + spec_terms + lookup_reps + (lookup_reps ? 1 : 0);
    return list_min(capacity, list_mul_add_sat(n, per_row, 0));
}

// The order of the list is kind 1, 2, 3, 4; the first min(capacity, total) entries are written.
struct ListSplit {
    uint64_t total;        // totals[0]: the sum of the four kinds (saturating; a sum of counts of one trace never does)
    uint64_t kept;         // entries written
    uint64_t first[5];     // [k]: position in the whole list of kind k's first entry, k = 1..4; [0] unused
    uint64_t written[5];   // [k]: entries of kind k among the kept ones; [0] = kept
};
inline ListSplit list_split(uint64_t capacity, const uint64_t totals_by_kind[5]) {
    ListSplit s{};
    uint64_t at = 0;
    for (int k = 1; k <= 4; k++) {
        s.first[k] = at;
        const uint64_t room = capacity > at ? capacity - at : 0;
        s.written[k] = list_min(room, totals_by_kind[k]);
        at = at > UINT64_MAX - totals_by_kind[k] ? UINT64_MAX : at + totals_by_kind[k];
    }
    s.total = at;
    s.kept = list_min(capacity, at);
    s.written[0] = s.kept;
    return s;
}

}  // namespace bj
