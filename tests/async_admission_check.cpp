// Stand-alone check of csrc/async_admission.h (tests/test_async_admission_host.py builds it with the address and undefined-behaviour
// sanitizers).  Shapes: the bench's SHA-256 geometry (workspace_plan_check.cpp) at 2^20 ... 2^24 rows, and at 2^10, 2^12 and 2^13
// rows, the circuits of tests/test_gpu_async_admission.py.  For each: every rung of the ladder is reached by some number of
// available bytes; each rung's threshold is exactly the bytes of its plan (one byte less picks the next rung); a lane that holds
// enough costs nothing; REFUSE only below the lean plan on one lane; a budget caps the free bytes by what is held; nothing wraps.
// Last, the condition the GPU test's budgets rest on: its slack is smaller than the gap to the next rung at the shapes it uses.
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

// The bench's geometry (60 general-purpose columns, 8 width-4 lookups, quotient degree 4; LDE 8, cap 16), a bj_prove that absorbs
// its column groups; `security` and the two public inputs as synthetic.sha_shaped_circuit has them for the small circuits.
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

static bj::AdmissionDecision decide(bj::AdmissionInput in, size_t available) {   // no budget: the free bytes are the available ones
    in.device_free = available, in.budget = 0;
    return bj::admit(in);
}

static void check_ladder(unsigned log_n, const bj::LaneBytes &res, const bj::LaneBytes &lean) {
    const size_t R = res.total(), Ln = lean.total();
    CHECK(Ln < R && R < ((size_t)1 << 48));
    CHECK(bj::grow_bytes(res, lean) == res.part[bj::LANE_ARENA] - lean.part[bj::LANE_ARENA]);   // the arena alone differs
    CHECK(bj::grow_bytes(lean, res) == 0 && bj::grow_bytes(res, res) == 0 && bj::grow_bytes(res, bj::LaneBytes()) == R);
    bj::AdmissionInput in;
    in.resident = res, in.lean = lean;
    bj::AdmissionDecision d;

    // nothing exists, nothing to release: resident from R on, lean from Ln on, refused below
    d = decide(in, R);
    CHECK(d.rung == bj::TWO_LANES_RESIDENT && d.lane == 0 && !d.lean && d.reserve_bytes == R && !d.wait && !d.release_parent);
    d = decide(in, R - 1);
    CHECK(d.rung == bj::LANE_LEAN && d.lane == 0 && d.lean && d.reserve_bytes == Ln);
    d = decide(in, Ln);
    CHECK(d.rung == bj::LANE_LEAN && d.want.total() == Ln);
    d = decide(in, Ln - 1);
    CHECK(d.rung == bj::REFUSE && d.reserve_bytes == Ln && d.available == Ln - 1);
    d = decide(in, 0);
    CHECK(d.rung == bj::REFUSE);

    // the parent holds a workspace and is idle: one lane once it has released it, resident if that fits; a busy parent releases nothing
    in.parent = res;
    const size_t back = res.releasable();
    CHECK(back > 0 && back < R);
    d = decide(in, Ln - 1);
    CHECK(d.rung == bj::ONE_LANE_AFTER_RELEASING_PARENT && d.release_parent && d.lane == 0 && d.available == Ln - 1 + back);
    CHECK(d.lean == (Ln - 1 + back < R));
    d = decide(in, R - back);
    CHECK(d.rung == bj::ONE_LANE_AFTER_RELEASING_PARENT && !d.lean && d.reserve_bytes == R);
    d = decide(in, R - back - 1);
    CHECK(d.rung == bj::ONE_LANE_AFTER_RELEASING_PARENT && d.lean);
    if (Ln > back) {
        d = decide(in, Ln - back);
        CHECK(d.rung == bj::ONE_LANE_AFTER_RELEASING_PARENT && d.lean);
        d = decide(in, Ln - back - 1);
        CHECK(d.rung == bj::REFUSE && d.available == Ln - 1);
    } else {
        d = decide(in, 0);
        CHECK(d.rung == bj::ONE_LANE_AFTER_RELEASING_PARENT);
    }
    in.parent_idle = false;
    d = decide(in, Ln - 1);
    CHECK(d.rung == bj::REFUSE && d.available == Ln - 1);
    in.parent_idle = true;

    // lane 0 exists, holds the resident footprint and is busy; the submission is due on lane 1
    in.created[0] = true, in.idle[0] = false, in.held[0] = res, in.due = 1;
    d = decide(in, R);
    CHECK(d.rung == bj::TWO_LANES_RESIDENT && d.lane == 1 && d.reserve_bytes == R && !d.wait);
    d = decide(in, R - 1);
    CHECK(d.rung == bj::LANE_LEAN && d.lane == 1 && d.reserve_bytes == Ln);
    d = decide(in, Ln);
    CHECK(d.rung == bj::LANE_LEAN);
    d = decide(in, Ln - 1);   // behind the lane that exists: it holds enough, so nothing is reserved and the parent keeps its workspace
    CHECK(d.rung == bj::ONE_LANE && d.lane == 0 && !d.lean && d.reserve_bytes == 0 && d.wait && !d.release_parent);
    d = decide(in, 0);
    CHECK(d.rung == bj::ONE_LANE && d.reserve_bytes == 0);
    CHECK(bj::admit(in, bj::ONE_LANE).rung == bj::ONE_LANE);   // asked again from a later rung (device_free 0)
    in.device_free = R;
    d = bj::admit(in, bj::LANE_LEAN);
    CHECK(d.rung == bj::LANE_LEAN && d.lane == 1);
    d = bj::admit(in, bj::ONE_LANE);
    CHECK(d.rung == bj::ONE_LANE && d.lane == 0);
    d = bj::admit(in, bj::REFUSE);
    CHECK(d.rung == bj::REFUSE);

    // due on lane 0 again, which holds enough: free of charge whatever is available
    in.due = 0, in.idle[0] = true;
    d = decide(in, 0);
    CHECK(d.rung == bj::TWO_LANES_RESIDENT && d.lane == 0 && d.reserve_bytes == 0);

    // lane 0 holds the lean footprint only, due on lane 1: behind lane 0, resident from exactly the arenas' difference on
    in.held[0] = lean, in.due = 1, in.parent = bj::LaneBytes();
    const size_t diff = bj::grow_bytes(res, lean);
    CHECK(diff < Ln || log_n > 0);
    if (diff < Ln) {
        d = decide(in, diff);
        CHECK(d.rung == bj::ONE_LANE && d.lane == 0 && !d.lean && d.reserve_bytes == diff);
        d = decide(in, diff - 1);
        CHECK(d.rung == bj::ONE_LANE && d.lane == 0 && d.lean && d.reserve_bytes == 0);
    } else {   // the lean lane of its own is cheaper than growing the other: the earlier rung wins from Ln on
        d = decide(in, Ln);
        CHECK(d.rung == bj::LANE_LEAN && d.lane == 1);
        d = decide(in, Ln - 1);
        CHECK(d.rung == bj::ONE_LANE && d.lean && d.reserve_bytes == 0);
    }
    // both lanes hold the lean footprint: lean for nothing, resident from the difference on
    in.created[1] = true, in.held[1] = lean;
    d = decide(in, diff - 1);
    CHECK(d.rung == bj::LANE_LEAN && d.lane == 1 && d.reserve_bytes == 0);
    d = decide(in, diff);
    CHECK(d.rung == bj::TWO_LANES_RESIDENT && d.lane == 1 && d.reserve_bytes == diff);

    // a budget: what is held comes off it, and it never raises what the device has free
    bj::AdmissionInput b;
    b.resident = res, b.lean = lean, b.parent = res, b.parent_idle = false;
    b.device_free = (size_t)288 << 30;
    b.budget = R + R;
    CHECK(b.available() == R && bj::admit(b).rung == bj::TWO_LANES_RESIDENT);
    b.budget = R + R - 1;
    CHECK(bj::admit(b).rung == bj::LANE_LEAN);
    b.budget = R + Ln - 1;
    CHECK(bj::admit(b).rung == bj::REFUSE);
    b.parent_idle = true;   // the parent's tables stay: they still count against the budget
    CHECK(b.available(true) == R + Ln - 1 - (R - back));
    b.budget = R - 1;       // below what is held already
    CHECK(b.available() == 0 && b.available(true) == back - 1);
    b.budget = R + R, b.device_free = Ln;
    CHECK(b.available() == Ln && bj::admit(b).rung == bj::LANE_LEAN);
    CHECK(bj::admission_available(5, 0, 1000) == 5 && bj::admission_available(5, 3, 1) == 2 && bj::admission_available(5, 3, 4) == 0);
}

int main() {
    size_t last = 0;
    for (unsigned log_n : {10u, 12u, 13u, 20u, 21u, 22u, 23u, 24u}) {
        const bj::WorkspaceShape s = shape_of(log_n, log_n < 20 ? 30 : 100, log_n < 20);
        const bj::LaneBytes res = bj::lane_footprint(s, false), lean = bj::lane_footprint(s, true);
        std::printf("log_n %2u: resident %zu bytes (arena %zu, staging %zu, scratch %zu, tables %zu), lean %zu (arena %zu)\n", log_n, res.total(),
                    res.part[bj::LANE_ARENA], res.part[bj::LANE_STAGING], res.part[bj::LANE_SCRATCH],
                    res.part[bj::LANE_TW_FWD] + res.part[bj::LANE_TW_INV] + res.part[bj::LANE_TW_SCALED22], lean.total(), lean.part[bj::LANE_ARENA]);
        CHECK(res.total() > last);   // grows with the trace: nothing wrapped
        last = res.total();
        CHECK(res.part[bj::LANE_STAGING] == (size_t)93 * 8 << log_n);
        CHECK(res.part[bj::LANE_SCRATCH] <= (size_t)8 << 27 && res.part[bj::LANE_SCRATCH] >= (size_t)8 * 8 << log_n);
        CHECK(res.part[bj::LANE_TW_FWD] == (size_t)4 * 8 << log_n);
        CHECK((res.part[bj::LANE_TW_SCALED22] != 0) == (log_n == 22));
        check_ladder(log_n, res, lean);
        // three footprints beside each other, as DESIGN.md §3 counts them: within 2^63 by a wide margin
        CHECK(3 * res.total() < ((size_t)1 << 50));
        if (log_n == 22) CHECK(res.part[bj::LANE_ARENA] > (size_t)62e9 && lean.part[bj::LANE_ARENA] < (size_t)27e9);
        // 2^23 rows beside the 75 GB setup on a 288 GB card: two resident lanes do not fit, a resident and a lean one do
        if (log_n == 23) CHECK(2 * res.total() > (size_t)(288e9 - 75e9) && res.total() + lean.total() < (size_t)(288e9 - 75e9));
        // The GPU test's budgets: H + R + Ln + 2 slack must stay below H + 2 R (2^13), H + R + slack below H + R + Ln and
        // tables + Ln + slack below R (2^12), slack being 16 MiB a lane: at most 2 MiB, the device allocator's block, over the
        // bytes counted for each of the eight device allocations a lane makes (arena, staging, scratch, three tables, its small
        // constants, its pointer table).
        const size_t slack = (size_t)16 << 20, tables = res.total() - res.releasable();
        if (log_n == 13) CHECK(2 * slack < res.total() - lean.total());
        if (log_n == 12) CHECK(slack < lean.total() && tables + lean.total() + slack < res.total());
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("async admission == expected\n");
    return 0;
}
