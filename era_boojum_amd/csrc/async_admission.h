// Admission of a bj_prove_async submission, defined once: given what the proof about to be submitted wants of a lane (its workspace
// plan resident and lean, workspace_plan.h, plus the lane's fixed extras), what the two lanes and the parent context already hold
// and the bytes available, which lane takes the proof, with which plan, and how many bytes that reserves.  The ladder, first rung
// that fits:
//   TWO_LANES_RESIDENT               the lane the submission is due on, resident workspace (what bj_prove_async always did);
//   LANE_LEAN                        that lane, lean workspace (BJ_PROOF_LEAN for this one proof: the same bytes, oracle_value.h);
//   ONE_LANE                         behind the other lane, which exists: resident if that fits, lean otherwise;
//   ONE_LANE_AFTER_RELEASING_PARENT  one lane as above, once the idle parent context has given its workspace back;
//   REFUSE                           not even the lean plan on one lane fits.
// A part of a lane (arena, staging, ...) that is already large enough costs nothing; one that is too small is freed and allocated
// again, so it costs the difference.  Plain C++17, no HIP: a host program can use it (tests/async_admission_check.cpp).
#pragma once
#include "workspace_plan.h"

#include <cstddef>
#include <cstdint>

namespace bj {

enum AdmissionRung : unsigned { TWO_LANES_RESIDENT = 0, LANE_LEAN, ONE_LANE, ONE_LANE_AFTER_RELEASING_PARENT, REFUSE };
inline const char *admission_name(unsigned rung) {
    static const char *const names[] = {"two lanes, resident", "lane lean", "one lane", "one lane after releasing the parent's workspace", "refused"};
    return rung <= REFUSE ? names[rung] : "?";
}

// What a context holds for proofs, in bytes, one number per device allocation (each grows by free and allocate).
enum LanePart : unsigned { LANE_ARENA, LANE_STAGING, LANE_SCRATCH, LANE_TW_FWD, LANE_TW_INV, LANE_TW_SCALED22, LANE_N_PARTS };
// bj_ctx_release_workspace gives the arena, the staging and the scratch back; the three tables stay
constexpr bool LANE_RELEASED[LANE_N_PARTS] = {true, true, true, false, false, false};
struct LaneBytes {
    size_t part[LANE_N_PARTS] = {};
    size_t total() const {
        size_t s = 0;
        for (size_t p : part) s += p;
        return s;
    }
    size_t releasable() const {   // what bj_ctx_release_workspace gives back
        size_t s = 0;
        for (unsigned i = 0; i < LANE_N_PARTS; i++)
            if (LANE_RELEASED[i]) s += part[i];
        return s;
    }
};
// bytes that bringing a context from `held` to at least `want` allocates
inline size_t grow_bytes(const LaneBytes &want, const LaneBytes &held) {
    size_t s = 0;
    for (unsigned i = 0; i < LANE_N_PARTS; i++)
        if (want.part[i] > held.part[i]) s += want.part[i] - held.part[i];
    return s;
}

// A twiddle table for 2^log_n points holds 2^(log_n - 1) words (one word below 2^1) and serves every smaller size as a prefix;
// twiddle_log: the smallest log_n whose table has at least `bytes`.
inline size_t twiddle_bytes(unsigned log_n) { return ((size_t)8 << (log_n ? log_n - 1 : 0)); }
inline unsigned twiddle_log(size_t bytes) {
    unsigned k = 1;
    while (twiddle_bytes(k) < bytes) k++;
    return k;
}

inline size_t intt_scratch_words(size_t len, size_t cols) {   // intt_groups (abi.hip): column groups whose scratch stays at 2^27 words
    const size_t cap = (size_t)1 << 27, group = len >= cap ? 1 : cap / len;
    return (cols < group ? cols : group) * len;
}
// The fixed extras of a context that proves shape `s` from a host witness: the staging of the witness columns with the
// multiplicity column behind them, the scratch of the widest inverse transform (upper bound: every witness or stage-2 column in one
// call, T's two columns on the quotient domain) and of the multiplicity count, both twiddle tables up to the LDE domain, and the
// scaled table of the tiled layout.  The arena is left 0.  A proof from values (s.n_values != 0, bj_prove_values) keeps all_values and
// the u32 multiplicity counters in the staging behind the multiplicity column: values_staging_bytes more, and nothing else moves.
inline size_t values_staging_bytes(size_t n, size_t n_values) { return n_values ? n_values * 8 + n * 4 : 0; }
inline LaneBytes lane_extras(const WorkspaceShape &s) {
    LaneBytes b;
    b.part[LANE_STAGING] = ((size_t)s.nW + (s.has_lookup ? 0 : 1)) * s.n * 8 + values_staging_bytes(s.n, s.n_values);
    size_t scratch = intt_scratch_words(s.n, s.nW > s.nS2 ? s.nW : s.nS2), t = intt_scratch_words(s.Q, 2);
    if (t > scratch) scratch = t;
    if (s.has_lookup && 2 * s.n + 2 > scratch) scratch = 2 * s.n + 2;
    b.part[LANE_SCRATCH] = scratch * 8;
    const size_t domain = s.Ln > s.N ? s.Ln : s.N;   // n times max(fri_lde, q), a power of two
    unsigned log_domain = 0;
    while (((size_t)1 << log_domain) < domain) log_domain++;
    b.part[LANE_TW_FWD] = b.part[LANE_TW_INV] = twiddle_bytes(log_domain);
    if (s.tiled) b.part[LANE_TW_SCALED22] = twiddle_bytes(22);
    return b;
}
// The footprint of a lane for shape `s` with the witness and stage-2 oracles resident or lean: the plan's total and the extras.
inline LaneBytes lane_footprint(WorkspaceShape s, bool lean_oracles) {
    s.lean_oracles = lean_oracles;
    LaneBytes b = lane_extras(s);
    b.part[LANE_ARENA] = workspace_plan(s).total() * 8;
    return b;
}

// The bytes that may still be allocated: the device's free bytes, capped by what a budget (BJ_HBM_BUDGET_BYTES, 0: none) leaves
// once the bytes the context and its lanes hold are taken off.
inline size_t admission_available(size_t device_free, size_t budget, size_t held_by_context_and_lanes) {
    if (!budget) return device_free;
    const size_t left = budget > held_by_context_and_lanes ? budget - held_by_context_and_lanes : 0;
    return left < device_free ? left : device_free;
}

struct AdmissionInput {
    LaneBytes resident, lean;      // what the submission wants of its lane, either way (equal where the proof is lean anyway)
    unsigned due = 0;              // the lane the submission is due on
    bool created[2] = {false, false};
    bool idle[2] = {true, true};   // no proof queued or running on it
    LaneBytes held[2];             // zero for a lane that does not exist
    LaneBytes parent;              // what the parent context holds
    bool parent_idle = true;
    size_t device_free = 0;        // hipMemGetInfo
    size_t budget = 0;             // BJ_HBM_BUDGET_BYTES
    size_t held_total() const { return parent.total() + held[0].total() + held[1].total(); }
    // bytes that may be allocated, now or once the parent has released its workspace
    size_t available(bool parent_released = false) const {
        const size_t back = parent_released ? parent.releasable() : 0;
        return admission_available(device_free + back, budget, held_total() - back);
    }
};
struct AdmissionDecision {
    AdmissionRung rung = REFUSE;
    unsigned lane = 0;
    bool lean = false;
    bool wait = false;             // the lane is busy: the submitter waits for it before it reserves
    bool release_parent = false;
    LaneBytes want;                // what the lane holds at least once the choice is carried out
    size_t reserve_bytes = 0;      // what carrying it out allocates (0: the lane holds enough); REFUSE: what the cheapest rung would
    size_t available = 0;          // the bytes the choice was measured against; REFUSE: the most any rung had
};

// first: the first rung tried (a caller whose reservation failed where the decision said it would fit asks again from the next)
inline AdmissionDecision admit(const AdmissionInput &in, unsigned first = TWO_LANES_RESIDENT) {
    AdmissionDecision d;
    const unsigned due = in.due & 1, other = due ^ 1;
    auto choose = [&](AdmissionRung rung, unsigned lane, bool lean, bool release) {
        const LaneBytes &want = lean ? in.lean : in.resident;
        const size_t need = grow_bytes(want, in.held[lane]), available = in.available(release);
        if (need > available) return false;
        d.rung = rung, d.lane = lane, d.lean = lean, d.wait = !in.idle[lane], d.release_parent = release, d.want = want;
        d.reserve_bytes = need, d.available = available;
        return true;
    };
    if (first <= TWO_LANES_RESIDENT && choose(TWO_LANES_RESIDENT, due, false, false)) return d;
    if (first <= LANE_LEAN && choose(LANE_LEAN, due, true, false)) return d;
    const unsigned one = in.created[other] ? other : due;   // the lane that exists
    if (first <= ONE_LANE && in.created[other] && (choose(ONE_LANE, other, false, false) || choose(ONE_LANE, other, true, false))) return d;
    const bool can_release = in.parent_idle && in.parent.releasable() != 0;
    if (first <= ONE_LANE_AFTER_RELEASING_PARENT && can_release &&
        (choose(ONE_LANE_AFTER_RELEASING_PARENT, one, false, true) || choose(ONE_LANE_AFTER_RELEASING_PARENT, one, true, true)))
        return d;
    d.rung = REFUSE, d.lane = one, d.lean = true, d.want = in.lean;
    d.reserve_bytes = grow_bytes(in.lean, in.held[one]);
    d.available = in.available(can_release);
    return d;
}

}  // namespace bj
