// witness_set_from_witness_vec (src/cs/implementations/witness.rs:386-443) on the device, from a setup's resident u32 placement:
// cell = all_values[placement[cell]], 0 for a placeholder.  A pure gather: per cell 4 bytes in, one random 8-byte read and 8 bytes
// out, so the random reads are what bounds it and the kernel is shaped to keep as many of them in flight as it can: a lane takes
// four consecutive cells with one 16-byte placement load, issues its four value loads before it uses any of them and writes two
// 16-byte stores; the grid is sized to the CU count (8 blocks of 256 threads per CU, every wave slot of a CU taken) and strides
// over the cells.  No LDS, vector stores only.  Nobody has measured other shapes: tools/prove_values_rate.py holds the figures.
// Also here: the u32 multiplicity counters of a WitnessVec widened into the [n] multiplicity column
// (materialize_multiplicities_polynomials, witness.rs:225-272).
#include "ctx.h"
#include "../../include/boojum_hip_diag.h"

using gl::u64;

namespace {

constexpr unsigned GATHER_THREADS = 256, GATHER_BLOCKS_PER_CU = 8, GATHER_CELLS_PER_LANE = 4;
constexpr uint32_t NONE = bj::PLACEMENT_NONE;

// The value of one cell.  A placeholder gives 0 without a load; an index at or beyond n_values gives 0 and raises *bad.
__device__ __forceinline__ u64 cell_value(uint32_t h, const u64 *__restrict__ values, size_t n_values, bool *bad) {
    if (h == NONE) return 0;
    if (h >= n_values) {
        *bad = true;
        return 0;
    }
    return values[h];
}

// quads: 4-cell groups the vector body takes (0 where a base is not 16-byte aligned); the cells from 4 * quads on go one by one
__global__ void __launch_bounds__(GATHER_THREADS)
witness_gather_kernel(const uint32_t *__restrict__ placement, const u64 *__restrict__ values, size_t n_values, u64 *__restrict__ cells,
                      size_t quads, size_t count, unsigned *bad_flag) {
    const size_t stride = (size_t)gridDim.x * GATHER_THREADS, first = (size_t)blockIdx.x * GATHER_THREADS + threadIdx.x;
    const uint4 *p4 = reinterpret_cast<const uint4 *>(placement);
    ulonglong2 *c2 = reinterpret_cast<ulonglong2 *>(cells);
    bool bad = false;
    for (size_t i = first; i < quads; i += stride) {
        const uint4 h = p4[i];
        // the four loads are independent and none is used before the stores below: they are in flight together
        const u64 v0 = cell_value(h.x, values, n_values, &bad), v1 = cell_value(h.y, values, n_values, &bad);
        const u64 v2 = cell_value(h.z, values, n_values, &bad), v3 = cell_value(h.w, values, n_values, &bad);
        c2[2 * i] = make_ulonglong2(v0, v1);
        c2[2 * i + 1] = make_ulonglong2(v2, v3);
    }
    for (size_t i = GATHER_CELLS_PER_LANE * quads + first; i < count; i += stride) cells[i] = cell_value(placement[i], values, n_values, &bad);
    // every lane is back here: one OR over the wave, one atomic from its first lane that saw a bad index
    const unsigned long long any = __ballot(bad);
    if (bad && (threadIdx.x & 63u) == (unsigned)(__ffsll((long long)any) - 1)) atomicOr(bad_flag, 1u);
}

__global__ void __launch_bounds__(256) widen_counters_kernel(const uint32_t *__restrict__ counters, size_t n_counters, u64 *__restrict__ column, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) column[i] = i < n_counters ? counters[i] : 0;
}

unsigned cu_count() {   // of the current device; 256 (an MI355X) where the runtime does not say
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        return 256;
    }
    return (unsigned)cus;
}

}  // namespace

namespace bj {

size_t witness_gather_sweep_cells() { return (size_t)cu_count() * GATHER_BLOCKS_PER_CU * GATHER_THREADS * GATHER_CELLS_PER_LANE; }

void launch_witness_gather(const uint32_t *d_placement, const u64 *d_values, size_t n_values, u64 *d_cells, size_t count, unsigned *d_bad,
                           hipStream_t s) {
    if (!count) return;
    // the column base c0 * n is 16-byte aligned only from n = 4 (placement) and n = 2 (cells) on: the vector body where both are
    const bool aligned = ((uintptr_t)d_placement | (uintptr_t)d_cells) % 16 == 0;
    const size_t quads = aligned ? count / GATHER_CELLS_PER_LANE : 0;
    const size_t lanes = quads > count - GATHER_CELLS_PER_LANE * quads ? quads : count - GATHER_CELLS_PER_LANE * quads;
    const size_t want = (lanes + GATHER_THREADS - 1) / GATHER_THREADS, most = (size_t)cu_count() * GATHER_BLOCKS_PER_CU;
    hipLaunchKernelGGL(witness_gather_kernel, dim3((unsigned)(want < most ? want : most)), dim3(GATHER_THREADS), 0, s, d_placement, d_values, n_values,
                       d_cells, quads, count, d_bad);
}

void launch_widen_counters(const uint32_t *d_counters, size_t n_counters, u64 *d_column, size_t n, hipStream_t s) {
    const size_t want = (n + 255) / 256, most = (size_t)cu_count() * GATHER_BLOCKS_PER_CU;
    hipLaunchKernelGGL(widen_counters_kernel, dim3((unsigned)(want < most ? want : most)), dim3(256), 0, s, d_counters, n_counters, d_column, n);
}

}  // namespace bj

// The test door of include/boojum_hip_diag.h: the kernel alone on caller-given device arrays.
extern "C" int bj_witness_gather(bj_ctx *ctx, const uint32_t *d_placement, unsigned cols, unsigned log_n, const uint64_t *d_values, size_t n_values,
                                 uint64_t *d_cells, unsigned *bad) {
    if (int rc = bj::bind(ctx)) return rc;
    if (!d_placement || !d_cells || !bad || (n_values && !d_values)) return bj::fail(ctx, BJ_ERR_INVALID_ARG, "bj_witness_gather: null pointer");
    if (log_n > 30 || ((uint64_t)cols << log_n) >= ((uint64_t)1 << 32))
        return bj::fail(ctx, BJ_ERR_UNSUPPORTED, "bj_witness_gather: %u columns of 2^%u rows (cols * n < 2^32, log_n <= 30)", cols, log_n);
    unsigned *d_bad = bj::values_bad_flag(ctx);
    BJ_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, ctx->stream));
    bj::launch_witness_gather(d_placement, d_values, n_values, d_cells, (size_t)cols << log_n, d_bad, ctx->stream);
    BJ_CHECK_LAUNCH(ctx);
    return bj_memcpy_d2h(ctx, bad, d_bad, 4);
}

extern "C" size_t bj_witness_gather_sweep_cells(bj_ctx *ctx) {
    if (bj::bind(ctx)) return 0;
    return bj::witness_gather_sweep_cells();
}
