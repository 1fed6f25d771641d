// Stand-alone check of csrc/ntt_plan.h (tests/test_ntt_plan_host.py builds it under the address and undefined-behaviour sanitizers):
// for every log_n 0..30 x {aligned, unaligned} x {two_pass on, off} the plan tiles the rounds [0, log_n), obeys the rules each
// kernel's launcher relies on, and is the row of the table below.  The table is the plan launch_ntt_passes ran before the plan
// became a value, recorded by running that function with every launch replaced by a print; it is literal on purpose.
// Then the launch arithmetic next to the plan: the columns per workgroup of the strided and local passes and the coset split of
// ntt_front10, for the wide-LDE shapes of tests/test_gpu_lde_cosets.py.
#include "ntt_plan.h"
#include "tiled_layout.h"

#include <cstdio>
#include <string>

using namespace bj;

// [log_n][0]: aligned with two_pass, [1]: aligned without, [2]: unaligned (with or without)
static const char *const TABLE[31][3] = {
    {"G0", "G0", "G0"},
    {"G1", "G1", "G1"},
    {"G2", "G2", "G2"},
    {"G3", "G3", "G3"},
    {"G4", "G4", "G4"},
    {"G5", "G5", "G5"},
    {"G6", "G6", "G6"},
    {"G7", "G7", "G7"},
    {"G8", "G8", "G8"},
    {"G9", "G9", "G9"},
    {"G10", "G10", "G10"},
    {"G11", "G11", "G11"},
    {"L12", "L12", "L12"},
    {"R1 L12", "R1 L12", "R1 L12"},
    {"F4 L10", "F4 L10", "F5 L9"},
    {"F5 L10", "F5 L10", "F5 L10"},
    {"S4 L12", "S4 L12", "S4 L12"},
    {"R1 S4 L12", "R1 S4 L12", "R1 S4 L12"},
    {"F4 S4 L10", "F4 S4 L10", "F5 S4 L9"},
    {"F5 S4 L10", "F5 S4 L10", "F5 S4 L10"},
    {"S8 L12", "S8 L12", "S8 L12"},
    {"R1 S8 L12", "R1 S8 L12", "R1 S8 L12"},
    {"F10 L12", "F4 S8 L10", "F5 S8 L9"},
    {"F5 S8 L10", "F5 S8 L10", "F5 S8 L10"},
    {"S8 S4 L12", "S8 S4 L12", "S8 S4 L12"},
    {"R1 S8 S4 L12", "R1 S8 S4 L12", "R1 S8 S4 L12"},
    {"F4 S8 S4 L10", "F4 S8 S4 L10", "F5 S8 S4 L9"},
    {"F5 S8 S4 L10", "F5 S8 S4 L10", "F5 S8 S4 L10"},
    {"S8 S8 L12", "S8 S8 L12", "S8 S8 L12"},
    {"R1 S8 S8 L12", "R1 S8 S8 L12", "R1 S8 S8 L12"},
    {"F4 S8 S8 L10", "F4 S8 S8 L10", "F5 S8 S8 L9"},
};

static int failures = 0;
#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            printf("log_n %u aligned %d two_pass %d pass %u: %s\n", sh.log_n, sh.aligned16, sh.two_pass, i, #cond);              \
            failures++;                                                                                                          \
        }                                                                                                                        \
    } while (0)

static std::string name(const NttPass &p) {
    switch (p.kind) {
    case NttPassKind::Generic: return "G" + std::to_string(p.rounds);
    case NttPassKind::FirstRound: return "R" + std::to_string(p.rounds);
    case NttPassKind::First4: return "F4";
    case NttPassKind::First5: return "F5";
    case NttPassKind::Front10: return "F10";
    case NttPassKind::Strided4: return "S4";
    case NttPassKind::Strided8: return "S8";
    case NttPassKind::Local: return "L" + std::to_string(p.rounds);
    }
    return "?";
}

static void check(const NttShape &sh) {
    const NttPlan plan = ntt_plan(sh);
    unsigned i = 0, r0 = 0;
    CHECK(plan.n_passes >= 1 && plan.n_passes <= 4);
    if (plan.n_passes < 1 || plan.n_passes > 4) return;
    std::string text;
    for (; i < plan.n_passes; i++) {
        const NttPass &p = plan.pass[i];
        const bool last = i + 1 == plan.n_passes;
        CHECK(p.r0 == r0);                                  // no gap, no overlap, in order
        CHECK(p.rounds >= 1 || sh.log_n == 0);
        switch (p.kind) {
        case NttPassKind::Generic: CHECK(sh.log_n < 12 && plan.n_passes == 1); break;
        case NttPassKind::FirstRound: CHECK(p.rounds == 1 && p.r0 == 0); break;
        case NttPassKind::First4: CHECK(p.rounds == 4 && i == 0 && sh.aligned16); break;
        case NttPassKind::First5: CHECK(p.rounds == 5 && i == 0); break;
        case NttPassKind::Front10: CHECK(p.rounds == 10 && i == 0 && sh.log_n == 22 && sh.aligned16 && sh.two_pass); break;
        // a strided workgroup owns 4096 elements, 2^rounds mid x 2^(12 - rounds) consecutive lo: the rounds from r0 on span >= 12 bits
        // (ntt_strided8 / ntt_strided4: rem_log = log_n - r0 - rounds >= 4 / >= 8)
        case NttPassKind::Strided4: CHECK(p.rounds == 4 && 12u + p.r0 <= sh.log_n); break;
        case NttPassKind::Strided8: CHECK(p.rounds == 8 && 12u + p.r0 <= sh.log_n); break;
        case NttPassKind::Local: CHECK(last && (p.rounds == 9 || p.rounds == 10 || p.rounds == 12)); break;
        }
        if (last && sh.log_n >= 12) CHECK(p.kind == NttPassKind::Local);
        r0 += p.rounds;
        text += (i ? " " : "") + name(p);
    }
    CHECK(r0 == sh.log_n);                                  // the passes cover every round
    const char *want = TABLE[sh.log_n][!sh.aligned16 ? 2 : sh.two_pass ? 0 : 1];
    if (text != want) {
        printf("log_n %u aligned %d two_pass %d: plan \"%s\", table \"%s\"\n", sh.log_n, sh.aligned16, sh.two_pass, text.c_str(), want);
        failures++;
    }
    CHECK(ntt_plan_is_two_pass(sh) == (text == "F10 L12"));
}

static std::string plan_text(const NttShape &sh) {
    const NttPlan plan = ntt_plan(sh);
    std::string text;
    for (unsigned i = 0; i < plan.n_passes; i++) text += (i ? " " : "") + name(plan.pass[i]);
    return text;
}

// The wide-LDE shapes of tests/test_gpu_lde_cosets.py that exist to run the column loop of a strided or local workgroup more than once
// (tests/lde_coset_shapes.py: MULTI_COLUMN; tests/test_ntt_plan_host.py compares the lines printed here with that list).  The GPU
// cannot show cols_per_block: the claim is kept here, literal, against pick_cols_per_block.
struct CpbCase {
    unsigned log_n;
    bool aligned;
    unsigned n_cols, n_cosets;
    const char *plan;
    unsigned cpb, groups, last;   // columns per workgroup, workgroups per tile and coset, columns of the last one
};
static const CpbCase CPB_CASES[] = {
    {12, true, 127, 64, "L12", 2, 64, 1},
    {18, true, 3, 64, "F4 S4 L10", 8, 1, 3},
    {18, false, 3, 64, "F5 S4 L9", 8, 1, 3},
    {17, true, 3, 64, "R1 S4 L12", 2, 2, 1},
};
// The same shapes at the coset counts the suite had before (at most 8): one column per workgroup, which is why the loop never ran twice.
static const CpbCase CPB_ONE[] = {
    {12, true, 127, 8, "L12", 1, 127, 1},
    {18, true, 3, 8, "F4 S4 L10", 1, 3, 1},
    {17, true, 3, 8, "R1 S4 L12", 1, 3, 1},
};

static void check_cpb(const CpbCase &c, bool print) {
    const NttShape sh{c.log_n, c.aligned, true};
    const unsigned i = 0;
    const unsigned tiles = 1u << (c.log_n - 12);   // launch_ntt_local12, launch_ntt_strided (ntt_r16.hip)
    const unsigned cpb = pick_cols_per_block(tiles, c.n_cols, c.n_cosets);
    const unsigned groups = (c.n_cols + cpb - 1) / cpb, last = c.n_cols - (groups - 1) * cpb;
    CHECK(plan_text(sh) == c.plan);
    CHECK(cpb == c.cpb);
    CHECK(groups == c.groups);
    CHECK(last == c.last);
    CHECK(last >= 1 && last <= cpb);
    if (print)
        printf("cpb log_n=%u aligned=%d n_cols=%u n_cosets=%u plan=\"%s\" cpb=%u groups=%u last=%u\n", c.log_n, c.aligned, c.n_cols, c.n_cosets,
               plan_text(sh).c_str(), cpb, groups, last);
}

// The launches of launch_ntt_front10 (ntt_r16.hip) for the three 2^22 cases (tests/lde_coset_shapes.py: FRONT10): its loop is
//     for (c0 = 0; c0 < n_cosets; c0 += FRONT10_COSETS_PER_LAUNCH) { nc = front10_launch_cosets(n_cosets, c0); cpb = front10_cols_per_block(tiles, n_cols, nc); ... }
// with tiles = 2^(12 - LB): LB = 4 for natural-order input (LBN there), TILED_LB for tiled input.
struct Front10Case {
    bool tiled;
    unsigned n_cols, n_cosets;
    const char *launches;   // "c0:nc:cpb,..."
};
static const Front10Case FRONT10_CASES[] = {
    {false, 1, 3, "0:3:1"},
    {false, 1, 9, "0:8:1,8:1:1"},
    {true, 1, 11, "0:8:8,8:3:1"},
};

static void check_front10(const Front10Case &c) {
    const NttShape sh{22, true, true};
    const unsigned i = 0;
    const unsigned tiles = 1u << (12 - (c.tiled ? TILED_LB : 4));
    std::string text;
    unsigned covered = 0;
    for (unsigned c0 = 0; c0 < c.n_cosets; c0 += FRONT10_COSETS_PER_LAUNCH) {
        const unsigned nc = front10_launch_cosets(c.n_cosets, c0);
        CHECK(nc >= 1 && nc <= 8 && c0 == covered);
        covered += nc;
        text += (c0 ? "," : "") + std::to_string(c0) + ":" + std::to_string(nc) + ":" + std::to_string(front10_cols_per_block(tiles, c.n_cols, nc));
    }
    CHECK(covered == c.n_cosets);
    CHECK(text == c.launches);
    CHECK(ntt_plan_is_two_pass(sh));
    printf("front10 tiled=%d n_cols=%u n_cosets=%u launches=%s\n", c.tiled, c.n_cols, c.n_cosets, text.c_str());
}

int main() {
    for (unsigned log_n = 0; log_n <= 30; log_n++)
        for (int aligned = 0; aligned < 2; aligned++)
            for (int two_pass = 0; two_pass < 2; two_pass++) check(NttShape{log_n, aligned != 0, two_pass != 0});

    for (const CpbCase &c : CPB_CASES) check_cpb(c, true);
    for (const CpbCase &c : CPB_ONE) check_cpb(c, false);
    for (const Front10Case &c : FRONT10_CASES) check_front10(c);
    {   // every launch of 1..64 cosets: whole launches of eight and one short one, in order, nothing left over
        const NttShape sh{22, true, true};
        unsigned i = 0;
        for (unsigned n_cosets = 1; n_cosets <= 64; n_cosets++) {
            unsigned covered = 0, launches = 0;
            for (unsigned c0 = 0; c0 < n_cosets; c0 += FRONT10_COSETS_PER_LAUNCH, launches++) covered += front10_launch_cosets(n_cosets, c0);
            CHECK(covered == n_cosets && launches == (n_cosets + 7) / 8);
        }
    }

    // ntt_aligned16: both pointers on 16-byte boundaries and both strides even
    alignas(16) static unsigned char buf[64];
    unsigned i = 0;
    const NttShape sh{0, false, false};
    CHECK(ntt_aligned16(buf, buf + 16, 4096, 8192));
    CHECK(!ntt_aligned16(buf + 8, buf + 16, 4096, 8192));
    CHECK(!ntt_aligned16(buf, buf + 8, 4096, 8192));
    CHECK(!ntt_aligned16(buf, buf + 16, 4097, 8192));
    CHECK(!ntt_aligned16(buf, buf + 16, 4096, 8193));

    if (failures) return 1;
    printf("ntt plan == table: 31 sizes x aligned x two_pass\n");
    return 0;
}
