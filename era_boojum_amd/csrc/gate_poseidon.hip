// Hand-written evaluators of the two flattened Poseidon gates for the quotient: Poseidon2FlattenedGate<8, 12, 4>, the gate of
// the recursion-layer circuits, and PoseidonFlattenedGate<8, 12, 4, PoseidonGoldilocks>, the Poseidon (v1) round-function gate
// circuits use to hash in-circuit.  The 118 terms of a repetition and their order are the walks of poseidon_gate_terms.h under
// the canonical-u64 policy.  The op-list interpreter (gate_program.hip) runs the same gates as 2.4 k (Poseidon2) and 3 457 (v1)
// recorded operations with their temporaries in scratch memory; here the state stays in registers and the terms go straight into
// the alpha-weighted gl::Acc160 accumulators (~10x fewer instructions per LDE point).  Same terms (as canonical residues), same
// order, same proof.
#include "gate_launch.h"
#include "gl.h"
#include "kernels.h"
#include "poseidon_gate_terms.h"

using gl::u64;

namespace bj {
namespace {

// out += selector * sum_t alpha_t * term_t at point I; KIND picks the walk
template <int KIND>
__device__ __forceinline__ void quotient_flattened(const u64 *vars, size_t var_stride, const u64 *consts, size_t const_stride,
                                                   unsigned path_len, unsigned path_bits, const u64 *alphas /* [118][2] */, size_t Q,
                                                   u64 *out0, u64 *out1) {
    const size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= Q) return;
    u64 sel = 1;
    for (unsigned b = 0; b < path_len; b++) {
        u64 c = gl::canon(consts[(size_t)b * const_stride + I]);
        sel = gl::mul(sel, ((path_bits >> b) & 1u) ? c : gl::sub(1, c));
    }
    gl::Acc160 a0, a1;
    a0.clear();
    a1.clear();
    unsigned term = 0;
    auto var = [&](unsigned k) { return gl::canon(vars[(size_t)k * var_stride + I]); };
    auto push = [&](u64 t) {
        a0.fma(t, alphas[2 * term]);
        a1.fma(t, alphas[2 * term + 1]);
        term++;
    };
    if constexpr (KIND == BJ_GATE_POSEIDON2_FLATTENED) poseidon2_flattened_terms<GateU64>(var, push);
    else poseidon1_flattened_terms<GateU64>(var, push);
    out0[I] = gl::add(gl::canon(out0[I]), gl::mul(a0.reduce(), sel));
    out1[I] = gl::add(gl::canon(out1[I]), gl::mul(a1.reduce(), sel));
}

__global__ void __launch_bounds__(256)
quotient_poseidon2_flattened_kernel(const u64 *vars, size_t var_stride, const u64 *consts, size_t const_stride,
                                    unsigned path_len, unsigned path_bits, const u64 *alphas, size_t Q, u64 *out0, u64 *out1) {
    quotient_flattened<BJ_GATE_POSEIDON2_FLATTENED>(vars, var_stride, consts, const_stride, path_len, path_bits, alphas, Q, out0, out1);
}
__global__ void __launch_bounds__(256)
quotient_poseidon_flattened_kernel(const u64 *vars, size_t var_stride, const u64 *consts, size_t const_stride,
                                   unsigned path_len, unsigned path_bits, const u64 *alphas, size_t Q, u64 *out0, u64 *out1) {
    quotient_flattened<BJ_GATE_POSEIDON_FLATTENED>(vars, var_stride, consts, const_stride, path_len, path_bits, alphas, Q, out0, out1);
}

}  // namespace

void launch_quotient_poseidon_gate(const GateShape &G, const GateCols &cols, const TermSink &out, hipStream_t s) {
    const auto kernel = G.kind == BJ_GATE_POSEIDON2_FLATTENED ? quotient_poseidon2_flattened_kernel : quotient_poseidon_flattened_kernel;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((out.points + 255) / 256)), dim3(256), 0, s, cols.vars.p, cols.vars.stride, cols.consts.p,
                       cols.consts.stride, G.path_len, path_bits(G), out.powers(G.first_term), out.points, out.out0, out.out1);
}

}  // namespace bj
