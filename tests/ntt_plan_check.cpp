// Stand-alone check of csrc/ntt_plan.h (tests/test_ntt_plan_host.py builds it under the address and undefined-behaviour sanitizers):
// for every log_n 0..30 x {aligned, unaligned} x {two_pass on, off} the plan tiles the rounds [0, log_n), obeys the rules each
// kernel's launcher relies on, and is the row of the table below.  The table is the plan launch_ntt_passes ran before the plan
// became a value, recorded by running that function with every launch replaced by a print; it is literal on purpose.
#include "ntt_plan.h"

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

int main() {
    for (unsigned log_n = 0; log_n <= 30; log_n++)
        for (int aligned = 0; aligned < 2; aligned++)
            for (int two_pass = 0; two_pass < 2; two_pass++) check(NttShape{log_n, aligned != 0, two_pass != 0});

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
