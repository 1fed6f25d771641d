// Internal: the index over the table rows of a lookup argument, shared by check_satisfied.hip (which compares the counts with a
// multiplicity column) and lookup_multiplicities.hip (which writes that column).  An open-addressing hash table of 2 n 32-bit
// slots over the n table rows: a slot holds SLOT_EMPTY or the smallest row of a class of equal rows (the all-zero padding rows
// are the large class), its representative.  lookup_build_kernel fills the slots (preset to 0xFF bytes); find_class probes them.
// Every cell is canonicalised as it is read.  Each including translation unit gets its own copy of the kernel.
#pragma once
#include "gl.h"

#include <hip/hip_runtime.h>

namespace bj {
namespace lookup {

using gl::u64;

constexpr unsigned INDEX_BLOCK = 256;       // threads per block of every kernel over the index
constexpr unsigned MAX_TUPLE = 16;          // lookup_width + 1 words held in registers
constexpr uint32_t SLOT_EMPTY = 0xFFFFFFFFu;
constexpr u64 NONE64 = ~0ull;

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }

// smallest key and number of the block's `bad` threads: one atomicMin and one atomicAdd per block that has any
__device__ __forceinline__ void block_min_count(bool bad, u64 key, u64 *out_min, u64 *out_cnt) {
    __shared__ u64 s_min[INDEX_BLOCK / 64];
    __shared__ unsigned s_cnt[INDEX_BLOCK / 64];
    u64 k = bad ? key : NONE64;
    const unsigned cnt = (unsigned)__popcll(__ballot(bad));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(k, off);
        k = o < k ? o : k;
    }
    if (lane_id() == 0) {
        s_min[threadIdx.x >> 6] = k;
        s_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 m = s_min[0];
        unsigned c = s_cnt[0];
#pragma unroll
        for (unsigned w = 1; w < INDEX_BLOCK / 64; w++) {
            m = s_min[w] < m ? s_min[w] : m;
            c += s_cnt[w];
        }
        if (c) {
            atomicMin((unsigned long long *)out_min, (unsigned long long)m);
            atomicAdd((unsigned long long *)out_cnt, (unsigned long long)c);
        }
    }
}

struct LookupShape {
    const u64 *tables;    // [w + 1][n] at tstride
    const u64 *lvars;     // [reps * cps][n] at vstride
    const u64 *table_id;  // [n], or nullptr: the id is the last variable column of the sub-argument
    size_t n, tstride, vstride;
    unsigned w, reps, cps, mask;   // mask: slots - 1
};

__device__ __forceinline__ uint32_t tuple_hash(const u64 *t, unsigned words) {
    u64 h = 0x9E3779B97F4A7C15ull;
    for (unsigned j = 0; j < words; j++) {
        h = (h ^ t[j]) * 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
    }
    h *= 0x94D049BB133111EBull;
    return (uint32_t)(h >> 32);
}
__device__ __forceinline__ void load_table_row(const LookupShape &L, size_t r, u64 *t) {
    for (unsigned j = 0; j <= L.w; j++) t[j] = gl::canon(L.tables[(size_t)j * L.tstride + r]);
}
// the tuple looked up by sub-argument `sub` on `row`: w cells, then the table id
__device__ __forceinline__ void load_looked_up(const LookupShape &L, size_t sub, size_t row, u64 *t) {
    for (unsigned j = 0; j < L.w; j++) t[j] = gl::canon(L.lvars[((size_t)sub * L.cps + j) * L.vstride + row]);
    t[L.w] = gl::canon(L.table_id ? L.table_id[row] : L.lvars[((size_t)sub * L.cps + L.w) * L.vstride + row]);
}
__device__ __forceinline__ bool table_row_equals(const LookupShape &L, size_t r, const u64 *t) {
    bool eq = true;
    for (unsigned j = 0; j <= L.w; j++) eq = eq && gl::canon(L.tables[(size_t)j * L.tstride + r]) == t[j];
    return eq;
}
__device__ __forceinline__ uint32_t slot_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// representative of the tuple's class, SLOT_EMPTY if no table row holds it (the table must be complete)
__device__ __forceinline__ uint32_t find_class(const LookupShape &L, const uint32_t *slots, const u64 *t) {
    uint32_t s = tuple_hash(t, L.w + 1) & L.mask;
    for (;;) {
        const uint32_t cur = slot_load(slots + s);
        if (cur == SLOT_EMPTY) return SLOT_EMPTY;
        if (table_row_equals(L, cur, t)) return cur;
        s = (s + 1) & L.mask;
    }
}

// one thread per table row: claim an empty slot, or lower the row number of the slot that holds an equal row.  The rows of a
// class (the all-zero padding rows are the large one) never probe past their class's slot, and only a row below the number
// they read there issues an atomic.
static __global__ void __launch_bounds__(INDEX_BLOCK) lookup_build_kernel(LookupShape L, uint32_t *slots) {
    const size_t r = (size_t)blockIdx.x * INDEX_BLOCK + threadIdx.x;
    if (r >= L.n) return;
    u64 t[MAX_TUPLE];
    load_table_row(L, r, t);
    uint32_t s = tuple_hash(t, L.w + 1) & L.mask;
    for (;;) {
        uint32_t cur = slot_load(slots + s);
        if (cur == SLOT_EMPTY) {
            cur = atomicCAS(slots + s, SLOT_EMPTY, (uint32_t)r);
            if (cur == SLOT_EMPTY) return;
        }
        if (table_row_equals(L, cur, t)) {
            if ((uint32_t)r < cur) atomicMin(slots + s, (uint32_t)r);
            return;
        }
        s = (s + 1) & L.mask;
    }
}

inline unsigned index_blocks(size_t items) { return (unsigned)((items + INDEX_BLOCK - 1) / INDEX_BLOCK); }

}  // namespace lookup
}  // namespace bj
