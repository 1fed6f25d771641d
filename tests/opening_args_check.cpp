// Stand-alone check of csrc/opening_args.h (tests/test_opening_args_host.py builds it host-only with the address and
// undefined-behaviour sanitizers): sources -> base columns with F_p^2 coefficients and the constant C of every set, against
// schoolbook F_p^2 arithmetic (u^2 = 7) on 128-bit integers written out here, and the recombination that inverts it.
// Nothing here touches a device: the pointers are host arrays used as addresses.
#include "opening_args.h"

#include <cstdio>
#include <random>

typedef uint64_t u64;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// the definition: residues as 128-bit integers reduced by %
static const u128 Pm = ((u128)1 << 64) - ((u128)1 << 32) + 1;
struct X2 { u128 a, b; };   // a + b u
static X2 x2(u64 a, u64 b) { return {a % Pm, b % Pm}; }
static X2 x2_add(X2 x, X2 y) { return {(x.a + y.a) % Pm, (x.b + y.b) % Pm}; }
static X2 x2_mul(X2 x, X2 y) { return {(x.a * y.a % Pm + 7 * (x.b * y.b % Pm)) % Pm, (x.a * y.b % Pm + x.b * y.a % Pm) % Pm}; }

static u64 cols[64][4];   // columns to point at, with values for the recombination check
static const u64 *col(int i) { return cols[i]; }

// One set of `srcs` appended to L must be: per source the column c0 with coefficient ch, then (F_p^2 source) the column c1 with
// coefficient u * ch; C = sum ch_k * v_k (0 without values); the point canonical
static void check_set(bj::ColumnList &L, const std::vector<bj::OpenSrc> &srcs, const std::vector<u64> &ch, const u64 *vals, const u64 *at) {
    const size_t first = L.n_cols(), set = L.sets.size();
    CHECK(L.add_set(srcs.data(), srcs.size(), ch.data(), vals, at));
    CHECK(L.ok && L.sets.size() == set + 1);
    if (L.sets.size() != set + 1) return;
    const bj::ColumnSet &S = L.sets[set];
    CHECK(S.first_col == first);
    size_t c = first;
    X2 C{0, 0};
    for (size_t k = 0; k < srcs.size(); k++) {
        const X2 chk = x2(ch[2 * k], ch[2 * k + 1]);
        if (vals) C = x2_add(C, x2_mul(chk, x2(vals[2 * k], vals[2 * k + 1])));
        CHECK(c < L.n_cols() && L.ptrs[c] == srcs[k].c0 && L.coefs[2 * c] == (u64)chk.a && L.coefs[2 * c + 1] == (u64)chk.b);
        c++;
        if (srcs[k].c1) {
            const X2 uch = x2_mul(chk, X2{0, 1});
            CHECK(c < L.n_cols() && L.ptrs[c] == srcs[k].c1 && L.coefs[2 * c] == (u64)uch.a && L.coefs[2 * c + 1] == (u64)uch.b);
            CHECK((u64)uch.a == (u64)(7 * chk.b % Pm) && (u64)uch.b == (u64)chk.a);   // the rule as the kernels' comment states it
            c++;
        }
    }
    CHECK(c == L.n_cols() && S.n_cols == c - first);
    CHECK(S.C[0] == (u64)C.a && S.C[1] == (u64)C.b);
    CHECK(S.at[0] == (u64)((at ? at[0] : 0) % Pm) && S.at[1] == (u64)((at ? at[1] : 0) % Pm));
    for (u64 w : L.coefs) CHECK(w < (u64)Pm);
    CHECK(L.coefs.size() == 2 * L.n_cols());
    CHECK(L.words() == bj::column_list_arg_words(L.n_cols()));
    CHECK(L.ptr_offset() == 0 && L.coef_offset() == L.n_cols());   // [pointers][coefficients] in one block
}

int main() {
    const u64 P = (u64)Pm, M = ~(u64)0;
    std::mt19937_64 rng(20250);
    for (auto &c : cols)
        for (u64 &w : c) w = rng();
    auto rnd = [&](size_t n) {
        std::vector<u64> v(n);
        for (u64 &w : v) w = rng();   // any u64: about one in 2^32 is non-canonical, the edge words below make sure of it
        return v;
    };
    const u64 edge[] = {P + 5, M, 0, P - 1, P, 1};

    // ---- base-only, F_p^2-only and mixed lists; three sets in one list ----
    {
        bj::ColumnList L;
        const std::vector<bj::OpenSrc> base = {{col(0), nullptr}, {col(1), nullptr}, {col(2), nullptr}};
        const std::vector<bj::OpenSrc> ext = {{col(3), col(4)}, {col(5), col(6)}};
        const std::vector<bj::OpenSrc> mixed = {{col(7), nullptr}, {col(8), col(9)}, {col(10), nullptr}, {col(11), col(12)}, {col(13), col(14)}};
        const u64 at0[2] = {P + 5, M}, at1[2] = {0, P - 1}, at2[2] = {rng(), rng()};
        const std::vector<u64> v0 = rnd(6), v1 = rnd(4), v2 = rnd(10);
        check_set(L, base, rnd(6), v0.data(), at0);
        check_set(L, ext, rnd(4), v1.data(), at1);
        check_set(L, mixed, rnd(10), v2.data(), at2);
        CHECK(L.sets.size() == 3 && L.n_cols() == 3 + 4 + 8);
        CHECK(L.sets[0].first_col == 0 && L.sets[0].n_cols == 3);
        CHECK(L.sets[1].first_col == 3 && L.sets[1].n_cols == 4);
        CHECK(L.sets[2].first_col == 7 && L.sets[2].n_cols == 8);
        CHECK(L.words() == 45);
    }
    // ---- challenges and values as non-canonical words: every pair of edge words in every position ----
    for (u64 a : edge)
        for (u64 b : edge)
            for (u64 c : edge)
                for (u64 d : edge) {
                    bj::ColumnList L;
                    const u64 at[2] = {b, c};
                    check_set(L, {{col(0), col(1)}, {col(2), nullptr}}, {a, b, c, d}, std::vector<u64>{c, d, a, b}.data(), at);
                    check_set(L, {{col(3), col(4)}}, {d, a}, nullptr, nullptr);   // no values, no point: bj_linear_combination
                    CHECK(L.sets.size() == 2 && L.sets[1].C[0] == 0 && L.sets[1].C[1] == 0);
                }
    // ---- random sets ----
    for (int it = 0; it < 200; it++) {
        bj::ColumnList L;
        std::vector<bj::OpenSrc> s(1 + rng() % 20);
        for (auto &x : s) x = {col(rng() % 64), rng() % 2 ? col(rng() % 64) : nullptr};
        const std::vector<u64> v = rnd(2 * s.size()), at = rnd(2);
        check_set(L, s, rnd(2 * s.size()), v.data(), at.data());
    }
    // ---- the C ABI's two arrays: a null c1 array against null entries inside it ----
    {
        const u64 *c0[3] = {col(0), col(1), col(2)}, *c1_none[3] = {nullptr, nullptr, nullptr}, *c1_some[3] = {nullptr, col(3), nullptr};
        const std::vector<bj::OpenSrc> a = bj::open_srcs(c0, nullptr, 3), b = bj::open_srcs(c0, c1_none, 3), c = bj::open_srcs(c0, c1_some, 3);
        for (int k = 0; k < 3; k++) {
            CHECK(a[k].c0 == c0[k] && a[k].c1 == nullptr && b[k].c0 == c0[k] && b[k].c1 == nullptr);
            CHECK(c[k].c0 == c0[k] && c[k].c1 == c1_some[k]);
        }
        const std::vector<u64> ch = rnd(6), v = rnd(6), at = rnd(2);
        bj::ColumnList La, Lb, Lc;
        check_set(La, a, ch, v.data(), at.data());
        check_set(Lb, b, ch, v.data(), at.data());
        check_set(Lc, c, ch, v.data(), at.data());
        CHECK(La.ptrs == Lb.ptrs && La.coefs == Lb.coefs && La.n_cols() == 3 && Lc.n_cols() == 4);
        CHECK(bj::open_srcs(c0, nullptr, 0).empty());
    }
    // ---- a source without a column: named by source and set, and the list stays unusable ----
    {
        bj::ColumnList L;
        const std::vector<u64> ch = rnd(6), v = rnd(6), at = rnd(2);
        check_set(L, {{col(0), nullptr}}, {ch[0], ch[1]}, v.data(), at.data());
        const std::vector<bj::OpenSrc> bad = {{col(1), col(2)}, {col(3), nullptr}, {nullptr, col(4)}};
        CHECK(!L.add_set(bad.data(), bad.size(), ch.data(), v.data(), at.data()));
        CHECK(!L.ok && L.bad_src == 2 && L.bad_set == 1 && L.sets.size() == 1);
        const bj::OpenSrc good{col(5), nullptr};
        CHECK(!L.add_set(&good, 1, ch.data(), v.data(), at.data()));   // no way back
        CHECK(!L.ok && L.bad_src == 2 && L.bad_set == 1 && L.sets.size() == 1);
        bj::ColumnList L0;
        const bj::OpenSrc none{nullptr, nullptr};
        CHECK(!L0.add_set(&none, 1, ch.data(), nullptr, nullptr) && L0.bad_src == 0 && L0.bad_set == 0 && L0.sets.empty());
    }
    // ---- the recombination inverts the flattening: evaluate every flattened column at an F_p^2 "weight", recombine, and
    //      compare with the F_p^2 polynomial (c0 + u c1) evaluated directly ----
    for (int it = 0; it < 200; it++) {
        std::vector<bj::OpenSrc> s(1 + rng() % 12);
        for (auto &x : s) x = {col(rng() % 64), rng() % 3 ? col(rng() % 64) : nullptr};
        const std::vector<const u64 *> flat_cols = bj::open_columns(s.data(), s.size());
        bj::ColumnList L;
        check_set(L, s, rnd(2 * s.size()), nullptr, nullptr);
        CHECK(flat_cols == L.ptrs);   // the same order as the flattening
        const std::vector<u64> w = rnd(8);   // four weights
        auto eval = [&](const u64 *f) {     // sum_i f[i] * w_i, as the barycentric kernels give it for a base column
            X2 e{0, 0};
            for (int i = 0; i < 4; i++) e = x2_add(e, x2_mul(x2(f[i], 0), x2(w[2 * i], w[2 * i + 1])));
            return e;
        };
        std::vector<u64> flat;
        for (const u64 *f : flat_cols) {
            const X2 e = eval(f);
            flat.push_back((u64)e.a + (it % 2 && e.a < ((u128)1 << 32) - 1 ? P : 0));   // now and then a non-canonical word
            flat.push_back((u64)e.b);
        }
        std::vector<u64> out(2 * s.size(), 12345);
        bj::recombine_values(s.data(), s.size(), flat.data(), out.data());
        for (size_t k = 0; k < s.size(); k++) {
            X2 want{0, 0};
            for (int i = 0; i < 4; i++)
                want = x2_add(want, x2_mul(x2(s[k].c0[i], s[k].c1 ? s[k].c1[i] : 0), x2(w[2 * i], w[2 * i + 1])));
            CHECK(out[2 * k] == (u64)want.a && out[2 * k + 1] == (u64)want.b);
        }
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("opening arguments == the definition\n");
    return 0;
}
