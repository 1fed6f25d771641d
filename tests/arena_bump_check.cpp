// Stand-alone check of csrc/arena_bump.h and of the twiddle_bytes / twiddle_log pair of csrc/async_admission.h
// (tests/test_arena_bump_host.py builds it with the address and undefined-behaviour sanitizers).  The placements at the edges of
// the arena, the 64-word alignment, the overflow slabs of a proof and what a request outside a proof gets; the high-water mark after
// every step of a sequence that mixes the three placements, against a transcription of the arithmetic the library's arena_alloc
// had before the header existed, on plain integers; reset; and the tables' bytes against lane_extras.
#include "arena_bump.h"
#include "async_admission.h"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

using bj::ArenaBump;

static ArenaBump arena_of(size_t words, size_t off = 0) {
    ArenaBump b;
    b.arena_words = words, b.arena_off = off;
    return b;
}
static bool same(const ArenaBump &a, const ArenaBump &b) {
    return a.arena_words == b.arena_words && a.arena_off == b.arena_off && a.slabs == b.slabs && a.slab_off == b.slab_off && a.high_water == b.high_water;
}

// arena_alloc as the library had it, line by line, with the device pointers left out: (base, elems) pairs became sizes, a returned
// pointer became (where, offset).  where: 0 nothing, 1 arena, 2 last slab, 3 new slab.
struct Before {
    size_t arena_elems = 0, arena_off = 0;
    std::vector<size_t> arena_slabs;
    size_t slab_off = 0, arena_high_water = 0;
    bool in_proof = false;
    std::pair<unsigned, size_t> arena_alloc(size_t elems) {
        const size_t start = (arena_off + 63) & ~(size_t)63;
        if (arena_slabs.empty() && start + elems <= arena_elems) {
            arena_off = start + elems;
            if (arena_off > arena_high_water) arena_high_water = arena_off;
            return {1, start};
        }
        if (!in_proof) return {0, 0};
        if (!arena_slabs.empty()) {
            size_t &last = arena_slabs.back();
            const size_t st = (slab_off + 63) & ~(size_t)63;
            if (st + elems <= last) {
                slab_off = st + elems;
                arena_high_water += elems + 64;
                return {2, st};
            }
        }
        const size_t slab = elems > ((size_t)1 << 25) ? elems : ((size_t)1 << 25);
        arena_slabs.emplace_back(slab);
        slab_off = elems;
        if (arena_high_water < arena_off) arena_high_water = arena_off;
        arena_high_water += elems + 64;
        return {3, 0};
    }
};

static void check_arena_placement() {
    ArenaBump b = arena_of(1000, 192);
    ArenaBump::Place at = b.place(808, false);   // ends exactly at the arena's last word
    CHECK(at.where == ArenaBump::ARENA && at.offset == 192 && b.arena_off == 1000 && b.high_water == 1000 && b.slabs.empty());
    b = arena_of(1000, 192);
    at = b.place(809, false);                    // one word longer
    CHECK(at.where == ArenaBump::NOTHING);
    b = arena_of(1000, 192);
    at = b.place(809, true);
    CHECK(at.where == ArenaBump::NEW_SLAB && b.arena_off == 192);
    for (size_t off : {(size_t)0, (size_t)64, (size_t)128}) {   // aligned starts stay
        b = arena_of(1000, off);
        CHECK(b.place(1, true).offset == off && b.arena_off == off + 1);
    }
    for (size_t off : {(size_t)1, (size_t)63}) {
        b = arena_of(1000, off);
        at = b.place(8, true);
        CHECK(at.where == ArenaBump::ARENA && at.offset == 64 && b.arena_off == 72);
    }
    b = arena_of(1000, 961);   // the rounded start, not the offset, decides: 1024 is past the end
    CHECK(b.place(1, false).where == ArenaBump::NOTHING);
    b = arena_of(0);
    at = b.place(0, false);    // nothing of nothing fits
    CHECK(at.where == ArenaBump::ARENA && at.offset == 0);
}

static void check_outside_a_proof() {
    ArenaBump b = arena_of(1000, 100);
    b.high_water = 100;
    const ArenaBump before = b;
    const ArenaBump::Place at = b.place(2000, false);
    CHECK(at.where == ArenaBump::NOTHING && same(b, before));
}

static void check_first_overflow_and_after() {
    const size_t MIN = (size_t)1 << 25;
    ArenaBump b = arena_of(1000, 0);
    ArenaBump::Place at = b.place(2000, true);   // the arena is empty and too small
    CHECK(at.where == ArenaBump::NEW_SLAB && at.offset == 0 && at.slab_words == MIN);
    CHECK(b.slabs.size() == 1 && b.slabs[0] == MIN && b.slab_off == 2000 && b.arena_off == 0 && b.high_water == 2064);
    at = b.place(10, true);                      // fits the arena, goes to the slab
    CHECK(at.where == ArenaBump::LAST_SLAB && at.offset == 2048 && b.slab_off == 2058 && b.arena_off == 0 && b.high_water == 2064 + 74);
    at = b.place(10, false);                     // outside a proof the slabs do not serve, and neither does the arena behind them
    CHECK(at.where == ArenaBump::NOTHING && b.slab_off == 2058 && b.arena_off == 0);
    at = b.place(MIN - 2112, true);              // ends exactly at the slab's last word
    CHECK(at.where == ArenaBump::LAST_SLAB && at.offset == 2112 && b.slab_off == MIN);
    at = b.place(1, true);                       // the slab is full
    CHECK(at.where == ArenaBump::NEW_SLAB && at.slab_words == MIN && b.slabs.size() == 2 && b.slab_off == 1);
    CHECK(b.slab_words() == 2 * MIN);

    b = arena_of(1000, 0);
    at = b.place(MIN, true);                     // 2^25 itself is the minimum
    CHECK(at.where == ArenaBump::NEW_SLAB && at.slab_words == MIN);
    b = arena_of(1000, 0);
    at = b.place(MIN + 1, true);                 // above it: exactly the request
    CHECK(at.where == ArenaBump::NEW_SLAB && at.slab_words == MIN + 1 && b.slabs[0] == MIN + 1 && b.slab_off == MIN + 1);
    at = b.place(1, true);                       // its rounded start is past the end
    CHECK(at.where == ArenaBump::NEW_SLAB && at.slab_words == MIN && b.slabs.size() == 2);

    b = arena_of(1000, 500);                     // the first slab raises the mark to the arena's offset first
    b.high_water = 0;
    at = b.place(600, true);
    CHECK(at.where == ArenaBump::NEW_SLAB && b.high_water == 500 + 600 + 64);
}

static void check_high_water_against_the_arithmetic_before() {
    const size_t MIN = (size_t)1 << 25;
    // (words, inside a proof): arena, arena after alignment, outside a proof and too large, the arena's exact end, first slab, last
    // slab three times, outside a proof with slabs open, a slab of the request's size, a slab because that one is full, last slab
    const std::pair<size_t, bool> steps[] = {{100, true}, {1, true},       {5000, false},  {808, true}, {10, true}, {5, true},
                                             {0, true},   {63, true},      {1, false},     {MIN + 7, true}, {3, true},  {MIN - 64, true},
                                             {64, true},  {2 * MIN, true}, {1, true}};
    ArenaBump b = arena_of(1000);
    Before ref;
    ref.arena_elems = 1000;
    unsigned seen[4] = {};
    for (const auto &st : steps) {
        ref.in_proof = st.second;
        const std::pair<unsigned, size_t> want = ref.arena_alloc(st.first);
        const ArenaBump::Place at = b.place(st.first, st.second);
        seen[want.first]++;
        CHECK((unsigned)at.where == want.first && at.offset == want.second);
        CHECK(b.high_water == ref.arena_high_water);
        CHECK(b.arena_off == ref.arena_off && b.slab_off == ref.slab_off && b.slabs == ref.arena_slabs);
        if (want.first == 3) CHECK(at.slab_words == ref.arena_slabs.back());
    }
    CHECK(seen[0] >= 2 && seen[1] >= 3 && seen[2] >= 4 && seen[3] >= 3);   // the sequence mixes every answer
    CHECK(b.high_water > 1000 && b.slabs.size() == seen[3]);

    b.reset();
    CHECK(b.arena_words == 1000 && b.arena_off == 0 && b.high_water == 0 && b.slabs.empty() && b.slab_off == 0);
    const ArenaBump::Place at = b.place(1000, false);   // the whole arena again
    CHECK(at.where == ArenaBump::ARENA && at.offset == 0 && b.high_water == 1000);
}

// the shapes of tests/async_admission_check.cpp: the bench's geometry at 2^10 ... 2^24 rows, LDE factor 8 against quotient degree 4,
// and the same with the domains of one rank of eight
static void check_twiddle_pair() {
    for (unsigned k = 1; k <= 32; k++) {
        CHECK(bj::twiddle_log(bj::twiddle_bytes(k)) == k);
        CHECK(bj::twiddle_bytes(k) == ((size_t)1 << (k - 1)) * 8);   // 2^(k-1) words
        if (k > 1) CHECK(bj::twiddle_log(bj::twiddle_bytes(k) - 1) == k && bj::twiddle_log(bj::twiddle_bytes(k - 1) + 1) == k);
    }
    CHECK(bj::twiddle_bytes(0) == 8 && bj::twiddle_log(0) == 1 && bj::twiddle_log(8) == 1);   // below 2^1: the table of 2^1
    for (unsigned log_n : {10u, 12u, 13u, 20u, 21u, 22u, 23u, 24u}) {
        bj_circuit ci{};
        ci.log_n = log_n; ci.num_gp_vars = 60; ci.num_vars = 92; ci.num_constant_cols = 8;
        ci.lookup_width = 4; ci.lookup_reps = 8; ci.table_id_col = 7; ci.quotient_degree = 4;
        bj_proof_config cfg{};
        cfg.fri_lde_factor = 8; cfg.cap_size = 16;
        const bj::ProofLayout layout = bj::proof_layout(bj::circuit_shape(&ci, &cfg));
        // lane_extras reads the sizes and widths alone: no FRI schedule, no public inputs
        bj::WorkspaceShape s = bj::workspace_shape(layout, 1, log_n == 22, 0, nullptr, nullptr, 0, false, bj::WS_HOST_ABSORBING, false, nullptr, 0, 0);
        CHECK(s.n == (size_t)1 << log_n && s.N == 8 * s.n && s.Ln == 8 * s.n);
        const bj::LaneBytes x = bj::lane_extras(s);
        CHECK(x.part[bj::LANE_TW_FWD] == bj::twiddle_bytes(log_n + 3) && x.part[bj::LANE_TW_INV] == bj::twiddle_bytes(log_n + 3));
        CHECK(x.part[bj::LANE_TW_FWD] == (size_t)4 * 8 << log_n);   // as async_admission_check.cpp states it
        CHECK(x.part[bj::LANE_TW_SCALED22] == (s.tiled ? bj::twiddle_bytes(22) : 0));
        CHECK(bj::twiddle_log(x.part[bj::LANE_TW_FWD]) == log_n + 3);
        s.N = 2 * s.n, s.Ln = s.n;   // a rank of eight: the larger of the two domains counts
        CHECK(bj::lane_extras(s).part[bj::LANE_TW_INV] == bj::twiddle_bytes(log_n + 1));
    }
    bj::WorkspaceShape tiny;   // the formula lane_extras had: (domain > 2 ? domain / 2 : 1) * 8
    for (size_t domain : {(size_t)1, (size_t)2, (size_t)4, (size_t)8}) {
        tiny.n = tiny.N = tiny.Ln = tiny.Q = domain, tiny.nW = 1;
        CHECK(bj::lane_extras(tiny).part[bj::LANE_TW_FWD] == (domain > 2 ? domain / 2 : 1) * 8);
    }
}

int main() {
    check_arena_placement();
    check_outside_a_proof();
    check_first_overflow_and_after();
    check_high_water_against_the_arithmetic_before();
    check_twiddle_pair();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("arena bump == expected\n");
    return 0;
}
