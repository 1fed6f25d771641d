// Stand-alone check of what bj_prove_values adds to csrc/async_admission.h (tests/test_prove_values_host.py builds it with the
// address and undefined-behaviour sanitizers): WorkspaceShape::n_values.  Shapes: those of tests/async_admission_check.cpp, the
// bench's SHA-256 geometry at 2^10, 2^12, 2^13 and 2^20 ... 2^24 rows.  With n_values == 0 (every caller there was before the
// field) lane_extras and lane_footprint give the numbers they gave: the parts restated here from their definition.  With n_values > 0
// the staging alone moves, by n_values * 8 + n * 4 bytes (all_values and the u32 counters behind the multiplicity column); the
// arena, the scratch and the tables do not, resident or lean, and the ladder admits by the larger footprint to the byte.
#include "async_admission.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// compute_fri_schedule (prover.rs:2281-2372) as bj_fri_schedule states it
static void schedule(unsigned security, size_t cap, unsigned pow_bits, unsigned rate_log2, unsigned deg, uint32_t *sched, size_t *len,
                     size_t *num_queries, unsigned *new_pow) {
    auto log2_of = [](size_t x) {
        unsigned r = 0;
        while (((size_t)1 << r) < x) r++;
        return r;
    };
    unsigned raw = security - pow_bits;
    *new_pow = pow_bits;
    if (raw % rate_log2 != 0 && *new_pow >= rate_log2 - raw % rate_log2) *new_pow -= rate_log2 - raw % rate_log2;
    raw = security - *new_pow;
    *num_queries = raw / rate_log2 + (raw % rate_log2 != 0 ? 1 : 0);
    const unsigned stop_log = log2_of(cap >> rate_log2 ? cap >> rate_log2 : 1), cap_log = log2_of(cap);
    *len = 0;
    while (deg > stop_log) {
        if (deg + rate_log2 <= cap_log) break;
        const unsigned gap = deg - stop_log, k = gap >= 3 ? 3 : gap;
        deg -= k;
        sched[(*len)++] = k;
        if ((k == 1 && gap == 1) || deg + rate_log2 <= cap_log) break;
    }
}

// 60 general-purpose columns, 8 width-4 lookups, quotient degree 4; LDE 8, cap 16; a proof that absorbs its column groups
static bj::WorkspaceShape shape_of(unsigned log_n, unsigned security, bool public_inputs) {
    bj_circuit ci{};
    ci.log_n = log_n; ci.num_gp_vars = 60; ci.num_vars = 92; ci.num_constant_cols = 8;
    ci.lookup_width = 4; ci.lookup_reps = 8; ci.table_id_col = 7; ci.quotient_degree = 4;
    bj_proof_config cfg{};
    cfg.fri_lde_factor = 8; cfg.cap_size = 16;
    const bj::ProofLayout layout = bj::proof_layout(bj::circuit_shape(&ci, &cfg));
    uint32_t sched[32];
    size_t len = 0, nq = 0;
    unsigned new_pow = 0;
    schedule(security, 16, 0, 3, log_n, sched, &len, &nq, &new_pow);
    const unsigned alpha_terms = layout.n_lookup_terms + 9 + 1 + layout.n_chunks;
    const unsigned pub_cols[2] = {0, 1}, pub_rows[2] = {0, 0};
    return bj::workspace_shape(layout, 1, log_n == 22, alpha_terms, pub_cols, pub_rows, public_inputs ? 2 : 0, false, bj::WS_HOST_ABSORBING,
                               new_pow != 0, sched, len, nq);
}

static bool same_but_staging(const bj::LaneBytes &a, const bj::LaneBytes &b) {
    for (unsigned p = 0; p < bj::LANE_N_PARTS; p++)
        if (p != bj::LANE_STAGING && a.part[p] != b.part[p]) return false;
    return true;
}

int main() {
    CHECK(bj::LANE_N_PARTS == 6);
    for (unsigned log_n : {10u, 12u, 13u, 20u, 21u, 22u, 23u, 24u}) {
        bj::WorkspaceShape s = shape_of(log_n, log_n < 20 ? 30 : 100, log_n < 20);
        const size_t n = (size_t)1 << log_n;
        CHECK(s.n_values == 0);   // the default: what every caller that does not know the field passes
        // n_values == 0: the parts as they were defined before the field existed.  93 columns of staging (92 variables and the
        // multiplicities); the scratch of the widest inverse transform, in groups that stay at 2^27 words (93 witness columns are
        // more than the stage-2 oracle's; T's two columns of 4 n points are fewer than 93 of n); tables of 8 n / 2 words
        const bj::LaneBytes x0 = bj::lane_extras(s);
        CHECK(x0.part[bj::LANE_ARENA] == 0);
        CHECK(x0.part[bj::LANE_STAGING] == 93 * n * 8);
        const size_t group = ((size_t)1 << 27) / n;
        CHECK(x0.part[bj::LANE_SCRATCH] == (93 < group ? 93 : group) * n * 8);
        CHECK(x0.part[bj::LANE_TW_FWD] == 8 * n / 2 * 8 && x0.part[bj::LANE_TW_INV] == 8 * n / 2 * 8);
        CHECK(x0.part[bj::LANE_TW_SCALED22] == (log_n == 22 ? ((size_t)1 << 21) * 8 : 0));
        for (bool lean : {false, true}) {
            bj::WorkspaceShape t = s;
            t.lean_oracles = lean;
            const bj::LaneBytes f0 = bj::lane_footprint(s, lean);
            CHECK(f0.part[bj::LANE_ARENA] == bj::workspace_plan(t).total() * 8 && same_but_staging(f0, [&] {
                bj::LaneBytes w = x0;
                w.part[bj::LANE_ARENA] = f0.part[bj::LANE_ARENA];
                return w;
            }()) && f0.part[bj::LANE_STAGING] == x0.part[bj::LANE_STAGING]);
        }
        // n_values > 0: the staging grows by n_values * 8 + n * 4, nothing else moves
        for (size_t n_values : {(size_t)1, (size_t)12345, 26 * n, ((size_t)1 << 32) - 1}) {
            bj::WorkspaceShape v = s;
            v.n_values = n_values;
            const bj::LaneBytes xv = bj::lane_extras(v);
            CHECK(same_but_staging(xv, x0));
            CHECK(xv.part[bj::LANE_STAGING] == x0.part[bj::LANE_STAGING] + n_values * 8 + n * 4);
            CHECK(xv.part[bj::LANE_STAGING] % 8 == 0);   // the staging is counted in words
            for (bool lean : {false, true}) {
                const bj::LaneBytes f0 = bj::lane_footprint(s, lean), fv = bj::lane_footprint(v, lean);
                CHECK(same_but_staging(fv, f0) && fv.total() == f0.total() + n_values * 8 + n * 4);
            }
            // admitted by that footprint to the byte: from nothing, the lean plan on one lane fits exactly its bytes
            bj::AdmissionInput in;
            in.resident = bj::lane_footprint(v, false), in.lean = bj::lane_footprint(v, true);
            in.device_free = in.lean.total();
            CHECK(bj::admit(in).rung == bj::LANE_LEAN && bj::admit(in).reserve_bytes == in.lean.total());
            in.device_free = in.lean.total() - 1;
            CHECK(bj::admit(in).rung == bj::REFUSE && bj::admit(in).reserve_bytes == in.lean.total());
            in.device_free = bj::lane_footprint(s, true).total();   // what a host-witness proof is admitted with is not enough
            CHECK(bj::admit(in).rung == bj::REFUSE);
        }
        std::printf("log_n %2u: staging %zu bytes, with 26 n values %zu\n", log_n, x0.part[bj::LANE_STAGING],
                    x0.part[bj::LANE_STAGING] + bj::values_staging_bytes(n, 26 * n));
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("prove-values admission == expected\n");
    return 0;
}
