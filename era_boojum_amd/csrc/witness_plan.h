// Internal: the column groups in which bj_prove brings a host witness over PCIe (prover.hip, round 1).  Pure host C++.
#pragma once
#include <vector>

namespace bj {
constexpr unsigned NO_ABSORB = ~0u;
struct WitnessGroup {
    unsigned c0, c1, absorb_from;   // columns [c0, c1); absorb_from == NO_ABSORB: no absorption after this group
};
// The plan: transfer / transform groups [c0, c1) with one event each, and after some of them one absorption run over the
// columns extended since the last one.  Nothing can be hashed before the first G columns have crossed PCIe, so those go in
// quarters (the transforms of a quarter run under the transfer of the next) and are absorbed together; from then on the
// transfer (PCIe, ~5 ms per 8 columns of 2^22 rows) runs ahead of the hashing (~10 ms), so the groups widen to 2 G and
// 3 G: fewer round trips of the 32-byte capacity per leaf and fewer launch tails.  `uniform` (BJ_PROVE_UNIFORM_GROUPS), or no
// absorption at all: equal groups of G columns.  At most 64 groups (one event each): G grows until the plan fits.
// nW: witness columns; G: columns per group, a multiple of 8 when `absorb`.
inline std::vector<WitnessGroup> host_witness_plan(unsigned nW, unsigned G, bool absorb, bool uniform) {
    std::vector<WitnessGroup> plan;
    for (;;) {
        plan.clear();
        if (!absorb || uniform) {
            for (unsigned c0 = 0; c0 < nW; c0 += G) plan.push_back({c0, c0 + G < nW ? c0 + G : nW, absorb ? c0 : NO_ABSORB});
        } else {
            const unsigned q = G / 4;   // G is a multiple of 8
            unsigned pos = 0;
            for (unsigned k = 0; k < 4 && pos < nW; k++) {
                const unsigned c1 = pos + q < nW ? pos + q : nW;
                plan.push_back({pos, c1, (k == 3 || c1 == nW) ? 0u : NO_ABSORB});
                pos = c1;
            }
            const unsigned widths[6] = {1, 2, 2, 3, 3, 3};
            for (unsigned k = 0; pos < nW; k++) {
                const unsigned w = G * widths[k < 6 ? k : 5];
                const unsigned c1 = pos + w < nW ? pos + w : nW;
                plan.push_back({pos, c1, pos});
                pos = c1;
            }
        }
        if (plan.size() <= 64) break;
        G = absorb ? G + 8 : G + 1;
    }
    return plan;
}
}  // namespace bj
