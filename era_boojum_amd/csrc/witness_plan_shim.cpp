// Test access to host_witness_plan (witness_plan.h).  Built into the host-only helper library alone (build.py:
// build_canon_helper), not into libboojum_hip.so: the public boundary does not grow by a test hook.
#include "witness_plan.h"

#include <cstddef>

// writes up to `cap` groups as (c0, c1, absorb_from) triples; returns the number of groups of the plan
extern "C" size_t bj_host_witness_plan(unsigned nW, unsigned G, int absorb, int uniform, unsigned *out3, size_t cap) {
    const std::vector<bj::WitnessGroup> plan = bj::host_witness_plan(nW, G, absorb != 0, uniform != 0);
    for (size_t i = 0; i < plan.size() && i < cap; i++) {
        out3[3 * i] = plan[i].c0;
        out3[3 * i + 1] = plan[i].c1;
        out3[3 * i + 2] = plan[i].absorb_from;
    }
    return plan.size();
}
