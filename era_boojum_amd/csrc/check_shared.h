// Internal: what bj_check_satisfied (check_satisfied.hip) and bj_list_unsatisfied (list_unsatisfied.hip) share, so that both
// flag the same rows and sum the same classes: the block size, the seed of the fixed weights, the kernel that sums a class's
// multiplicities.  Each including translation unit gets its own copy of the kernel, as with lookup_index.h.
#pragma once
#include "lookup_index.h"

namespace bj {
namespace check {

using gl::u64;
using namespace bj::lookup;

constexpr unsigned CHECK_BLOCK = bj::lookup::INDEX_BLOCK;   // threads per block of every kernel here; also the points a row is replicated over
constexpr u64 ALPHA_SEED = 0x626A5F636865636Bull;   // "bj_check" (include/boojum_hip.h)

// one thread per table row: remember its class, add its canonical multiplicity to the class's 96-bit sum (lo, carries in hi)
static __global__ void __launch_bounds__(CHECK_BLOCK) lookup_expected_kernel(LookupShape L, const uint32_t *slots, const u64 *mult, uint32_t *class_of,
                                                                     unsigned long long *lo, uint32_t *hi) {
    const size_t r = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    if (r >= L.n) return;
    u64 t[MAX_TUPLE];
    load_table_row(L, r, t);
    const uint32_t cls = find_class(L, slots, t);
    class_of[r] = cls;
    const u64 m = gl::canon(mult[r]);
    if (m) {
        const u64 old = atomicAdd(lo + cls, (unsigned long long)m);
        if (old + m < old) atomicAdd(hi + cls, 1u);
    }
}

__host__ __device__ __forceinline__ u64 expected_value(u64 lo, uint32_t hi) { return gl::canon(gl::reduce128((u64)hi, lo)); }

inline u64 splitmix64(u64 &state) {
    u64 z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline unsigned blocks_for(size_t items) { return (unsigned)((items + CHECK_BLOCK - 1) / CHECK_BLOCK); }

}  // namespace check
}  // namespace bj
