// Test access to host_witness_plan (witness_plan.h) and to the workspace plan of a proof (workspace_plan.h).  Built into the host-only helper library alone (build.py:
// build_canon_helper), not into libboojum_hip.so: the public boundary does not grow by a test hook.
#include "witness_plan.h"
#include "workspace_plan.h"

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

// The workspace plan of a proof.  circuit9: log_n, num_vars, num_gp_vars, num_witness_cols, num_constant_cols, lookup_width,
// lookup_reps, table_id_col, quotient_degree; flags4: tiled (bit 0; bit 1: a lean setup, bit 2: a lean proof), multiplicity column
// counted into the arena, host-witness mode (0 none, 1 absorbing, 2 not absorbing), proof of work; sched / num_queries:
// bj_fri_schedule of the proof config.
// out4: total words, words of the allowance entries, number of entries, words of the exact entries.
extern "C" void bj_workspace_plan_summary(const unsigned *circuit9, unsigned fri_lde, unsigned cap_size, unsigned world, unsigned alpha_terms,
                                          const unsigned *pub_cols, const unsigned *pub_rows, size_t n_pub, const unsigned *flags4,
                                          const uint32_t *sched, size_t sched_len, size_t num_queries, size_t *out4) {
    bj_circuit c{};
    c.log_n = circuit9[0]; c.num_vars = circuit9[1]; c.num_gp_vars = circuit9[2]; c.num_witness_cols = circuit9[3];
    c.num_constant_cols = circuit9[4]; c.lookup_width = circuit9[5]; c.lookup_reps = circuit9[6]; c.table_id_col = circuit9[7];
    c.quotient_degree = circuit9[8];
    bj_proof_config cfg{};
    cfg.fri_lde_factor = fri_lde; cfg.cap_size = cap_size;
    const bj::ProofLayout L = bj::proof_layout(bj::circuit_shape(&c, &cfg));
    bj::WorkspaceShape s = bj::workspace_shape(L, world, (flags4[0] & 1) != 0, alpha_terms, pub_cols, pub_rows, n_pub, flags4[1] != 0, flags4[2],
                                               flags4[3] != 0, sched, sched_len, num_queries);
    s.lean = (flags4[0] & 2) != 0, s.lean_oracles = (flags4[0] & 4) != 0;
    const bj::WorkspacePlan P = bj::workspace_plan(s);
    size_t exact = 0;
    for (const bj::WorkspaceEntry &e : P.entries)
        if (e.exact) exact += e.words;
    out4[0] = P.total(), out4[1] = P.allowance_words(), out4[2] = P.entries.size(), out4[3] = exact;
}
