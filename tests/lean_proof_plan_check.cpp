// Stand-alone check of the lean-proof side of csrc/workspace_plan.h (WorkspaceShape::lean_oracles, BJ_PROOF_LEAN;
// tests/test_lean_proof_plan_host.py builds it with the address and undefined-behaviour sanitizers).  Two shapes on one GPU, LDE 8,
// cap 16, 100 bits, quotient degree 4:
//   A  2^10 rows, the bench's SHA-256 geometry with lookups (92 variables, 8 width-4 lookups) and one public input, witness resident;
//   B  2^12 rows, 60 variables, no lookups, no public input, witness from the host, absorbed in groups.
// With lean_oracles: wit_lde and s2_lde are one coset (nW n and nS2 n words), there are no capacity words, every opening set has
// its extended numerator, and the total is below the resident total by at least (nW + nS2) (Ln - n) - 2 N S words (S opening
// sets).  Without: the plan is, entry for entry, the plan this header made before it knew the flag — the tables below are that
// header's output for the two shapes, recorded; the widths and counts are written out from the circuits' numbers.
#include "workspace_plan.h"

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

struct Recorded {
    unsigned id;
    size_t words;
    int exact;
    size_t offset;
};
// id numbers as in the WsId enum: 1 wit_lde, 2 mono, 3 mono_s2, 4 wit_tree, 5 capacity, 6 s2_nat, 7 stage-2 scratch, 8 s2_lde, 9 s2_tree, ...
static const Recorded RESIDENT_A[] = {
    {1, 761856, 1, 0},        {2, 95232, 1, 761856},    {3, 65536, 1, 857088},    {4, 65472, 1, 922624},    {6, 65536, 1, 988096},
    {7, 47122, 1, 1053632},   {8, 524288, 1, 1100800},  {9, 65472, 1, 1625088},   {10, 84, 1, 1690560},     {11, 8192, 1, 1690688},
    {16, 65536, 1, 1698880},  {17, 65472, 1, 1764416},  {18, 2048, 1, 1829888},   {33, 1350, 0, 1831936},   {33, 10, 0, 1833344},
    {33, 90, 0, 1833408},     {19, 16384, 1, 1833536},  {20, 2048, 1, 1849920},   {22, 16384, 1, 1851968},  {34, 810, 0, 1868352},
    {22, 16384, 1, 1869184},  {34, 54, 0, 1885568},     {35, 18, 0, 1885632},     {35, 3, 0, 1885696},      {23, 8128, 1, 1885760},
    {24, 2048, 1, 1893888},   {23, 960, 1, 1895936},    {24, 256, 1, 1896896},    {23, 64, 1, 1897152},     {24, 32, 1, 1897216},
    {26, 32, 1, 1897280},     {28, 34, 1, 1897344},     {29, 14076, 1, 1897408},  {31, 34, 1, 1911488},     {32, 2720, 1, 1911552},
};
static const Recorded RESIDENT_B[] = {
    {1, 1966080, 1, 0},       {2, 245760, 1, 1966080},  {3, 122880, 1, 2211840},  {4, 262080, 1, 2334720},  {5, 131072, 1, 2596800},
    {6, 122880, 1, 2727872},  {7, 122904, 1, 2850752},  {8, 983040, 1, 2973696},  {9, 262080, 1, 3956736},  {10, 50, 1, 4218816},
    {11, 32768, 1, 4218880},  {16, 262144, 1, 4251648}, {17, 262080, 1, 4513792}, {18, 8192, 1, 4775872},   {33, 825, 0, 4784064},
    {33, 10, 0, 4784896},     {19, 65536, 1, 4784960},  {20, 8192, 1, 4850496},   {22, 65536, 1, 4858688},  {34, 495, 0, 4924224},
    {35, 12, 0, 4924736},     {23, 32704, 1, 4924800},  {24, 8192, 1, 4957504},   {23, 4032, 1, 4965696},   {24, 1024, 1, 4969728},
    {23, 448, 1, 4970752},    {24, 128, 1, 4971200},    {23, 64, 1, 4971328},     {24, 32, 1, 4971392},     {26, 32, 1, 4971456},
    {28, 34, 1, 4971520},     {29, 11594, 1, 4971584},  {31, 34, 1, 4983232},     {32, 3264, 1, 4983296},
};

// compute_fri_schedule (prover.rs:2281-2372) as bj_fri_schedule states it, without proof of work
static void schedule(unsigned security, size_t cap, unsigned rate_log2, unsigned deg, uint32_t *sched, size_t *len, size_t *num_queries) {
    auto log2_of = [](size_t x) {
        unsigned r = 0;
        while (((size_t)1 << r) < x) r++;
        return r;
    };
    *num_queries = security / rate_log2 + (security % rate_log2 != 0 ? 1 : 0);
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

static bj::WorkspaceShape shape_of(bool lookups, unsigned log_n) {
    bj_circuit ci{};
    ci.log_n = log_n; ci.num_gp_vars = 60; ci.num_vars = lookups ? 92 : 60; ci.num_constant_cols = lookups ? 8 : 7;
    ci.lookup_width = lookups ? 4 : 0; ci.lookup_reps = lookups ? 8 : 0; ci.table_id_col = lookups ? 7 : 0; ci.quotient_degree = 4;
    bj_proof_config cfg{};
    cfg.fri_lde_factor = 8; cfg.cap_size = 16;
    const bj::ProofLayout L = bj::proof_layout(bj::circuit_shape(&ci, &cfg));
    uint32_t sched[32];
    size_t len = 0, nq = 0;
    schedule(100, 16, 3, log_n, sched, &len, &nq);
    const unsigned pub_col[1] = {3}, pub_row[1] = {5};
    return bj::workspace_shape(L, 1, false, L.n_lookup_terms + 9 + 1 + L.n_chunks, pub_col, pub_row, lookups ? 1 : 0, false,
                               lookups ? bj::WS_HOST_NONE : bj::WS_HOST_ABSORBING, false, sched, len, nq);
}

// nW, nS2: the leaf widths from the circuit's numbers (variables + multiplicity column; z, the partial products of ceil(V / q)
// chunks and the lookup sums, two columns each); sets: everything at z, z(x) at z omega, the lookup sums at 0, the public input's row
static void check(const char *name, bool lookups, unsigned log_n, const Recorded *recorded, size_t n_recorded, size_t nW, size_t nS2, size_t sets,
                  size_t sets_large_resident) {
    const size_t n = (size_t)1 << log_n, N = 8 * n, Ln = 8 * n;   // LDE 8 >= quotient degree 4: the FRI domain is the LDE
    bj::WorkspaceShape s = shape_of(lookups, log_n);
    CHECK(s.nW == nW && s.nS2 == nS2 && s.N == N && s.Ln == Ln && !s.lean_oracles);
    // flag off: the recorded plan
    const bj::WorkspacePlan R = bj::workspace_plan(s);
    CHECK(R.entries.size() == n_recorded);
    size_t num_lde = 0;
    for (size_t i = 0; i < R.entries.size() && i < n_recorded; i++) {
        const bj::WorkspaceEntry &e = R.entries[i];
        CHECK((unsigned)e.id == recorded[i].id && e.words == recorded[i].words && (int)e.exact == recorded[i].exact && e.offset == recorded[i].offset);
        if (e.id == bj::WS_WIT_LDE) CHECK(e.words == nW * Ln);
        if (e.id == bj::WS_S2_LDE) CHECK(e.words == nS2 * Ln);
        if (e.id == bj::WS_CAPACITY) CHECK(e.words == 4 * N && !lookups);
        num_lde += e.id == bj::WS_NUM_LDE;
    }
    CHECK(num_lde == sets_large_resident);
    // flag on
    s.lean_oracles = true;
    const bj::WorkspacePlan P = bj::workspace_plan(s);
    size_t wit = 0, s2 = 0, end = 0;
    num_lde = 0;
    size_t combine = 0;
    for (const bj::WorkspaceEntry &e : P.entries) {
        CHECK(e.offset % bj::WS_ALIGN == 0 && e.offset >= end && e.offset < end + bj::WS_ALIGN && e.words > 0);
        end = e.offset + e.words;
        CHECK(e.id != bj::WS_CAPACITY);
        wit += e.id == bj::WS_WIT_LDE, s2 += e.id == bj::WS_S2_LDE, num_lde += e.id == bj::WS_NUM_LDE, combine += e.id == bj::WS_ARGS_COMBINE;
        if (e.id == bj::WS_WIT_LDE) CHECK(e.exact && e.words == nW * n);
        if (e.id == bj::WS_S2_LDE) CHECK(e.exact && e.words == nS2 * n);
        if (e.id == bj::WS_NUM_LDE) CHECK(e.exact && e.words == 2 * N);
        if (e.id == bj::WS_ARGS_COMBINE) CHECK(!e.exact);
        if (e.id == bj::WS_MONO) CHECK(e.words == nW * n);
        if (e.id == bj::WS_MONO_S2) CHECK(e.words == nS2 * n);
        if (e.id == bj::WS_WIT_TREE || e.id == bj::WS_S2_TREE) CHECK(e.words == (2 * N - 16) * 4);
    }
    CHECK(P.total() == end && wit == 1 && s2 == 1);
    CHECK(num_lde == sets && combine == sets);
    const size_t bound = (nW + nS2) * (Ln - n) - 2 * N * sets;
    CHECK(recorded[n_recorded - 1].offset + recorded[n_recorded - 1].words == R.total());
    CHECK(P.total() + bound <= R.total());
    // and with a lean setup as well: its coset buffer more, the same set rule
    s.lean = true;
    const bj::WorkspacePlan PL = bj::workspace_plan(s);
    num_lde = 0;
    for (const bj::WorkspaceEntry &e : PL.entries) num_lde += e.id == bj::WS_NUM_LDE;
    CHECK(num_lde == sets && PL.entries.size() == P.entries.size() + 1);
    std::printf("%s: resident %zu words, lean %zu words, saved %zu >= bound %zu\n", name, R.total(), P.total(), R.total() - P.total(), bound);
}

int main() {
    check("A", true, 10, RESIDENT_A, sizeof RESIDENT_A / sizeof *RESIDENT_A, 92 + 1, 2 * (1 + (92 / 4 - 1) + (8 + 1)), 4, 2);
    check("B", false, 12, RESIDENT_B, sizeof RESIDENT_B / sizeof *RESIDENT_B, 60, 2 * (1 + (60 / 4 - 1)), 2, 1);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("lean proof plan == expected\n");
    return 0;
}
