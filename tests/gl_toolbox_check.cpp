// Host check of the shared field helpers of csrc/gl.h — gl::Acc160, Acc160x2, inv_chain, e2_inv_chain, mul7, pow7, omega_pow_nat,
// domain_point, reduce128 — against unsigned __int128 arithmetic mod p and against gl::pow / gl::inv / gl::e2_mul / gl::e2_inv.  They are
// __host__ __device__; tests/test_gl_toolbox_host.py builds this file for the host with the address and undefined-behaviour
// sanitizers and runs it.  The kernels that use the helpers are compared with independent references by the GPU tests.
#include "gl.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

static int checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        checks++;                                         \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            exit(1);                                      \
        }                                                 \
    } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u64 rnd() {   // splitmix64
    u64 z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static u64 rnd_canon() { return rnd() % gl::P; }
static u64 rnd_word() {   // any u64; a quarter of them in [p, 2^64)
    const u64 r = rnd();
    return (r & 3) == 0 ? gl::P + (r >> 32) % 0xFFFFFFFFULL : rnd();
}
static u64 mulmod(u64 a, u64 b) { return (u64)((u128)a * b % gl::P); }
static u64 addmod(u64 a, u64 b) { return (u64)(((u128)a + b) % gl::P); }

// gl::reduce128 on the grid that tests/field_helper_cases.py gives the device: both limbs of the high word on their edges, the
// low word on the edge words and where the intermediate sum r lands on p - 1, p, p + 1, 2^64 - 1 and wraps to 0 and 1 (with
// and without the first step's borrow)
static void check_reduce128_grid() {
    const u64 P = gl::P, E = gl::EPS;
    const u64 limbs[] = {0, 1, 2, 0x7FFFFFFFULL, 0x80000000ULL, 0xFFFFFFFEULL, 0xFFFFFFFFULL};
    const u64 words[] = {0, 1, 2, 7, 1ULL << 16, E, E + 1, E + 2, 1ULL << 48, (1ULL << 48) - 1, P - 2, P - 1, P, P + 1, ~0ULL - E, ~0ULL - 1,
                         ~0ULL, 1ULL << 63, (1ULL << 63) - 1, 0xFFFFFFFF00000000ULL, 0xFFFFFFFEFFFFFFFFULL, 0xFFFFFFFE00000001ULL,
                         0x8000000080000000ULL, 0x00000001FFFFFFFFULL};
    const u64 targets[] = {P - 1, P, P + 1, ~0ULL, 0, 1};   // mod 2^64
    for (u64 hh : limbs)
        for (u64 hl : limbs) {
            std::vector<u64> los(words, words + sizeof(words) / sizeof(words[0]));
            for (u64 t : targets) {
                los.push_back(t - hl * E + hh);
                los.push_back(t - hl * E + hh + E);
            }
            for (u64 lo : los) {
                const u64 hi = (hh << 32) | hl, got = gl::reduce128(hi, lo);
                const u64 want = (u64)((((u128)hi << 64) | lo) % P);
                CHECK(got == want, "reduce128(%016llx, %016llx) = %016llx, not %016llx", (unsigned long long)hi, (unsigned long long)lo,
                      (unsigned long long)got, (unsigned long long)want);
                CHECK(gl::reduce_limbs((u32)hh, (u32)hl, lo) == want, "reduce_limbs(%08x, %08x, %016llx)", (u32)hh, (u32)hl, (unsigned long long)lo);
            }
        }
    for (int i = 0; i < 20000; i++) {
        const u64 hi = rnd(), lo = rnd();
        CHECK(gl::reduce128(hi, lo) == (u64)((((u128)hi << 64) | lo) % P), "reduce128(%016llx, %016llx)", (unsigned long long)hi, (unsigned long long)lo);
    }
}

static void check_acc160() {
    const int ks[] = {1, 2, 5, 118, 4096};
    for (int all_ones = 0; all_ones < 2; all_ones++)
        for (int k : ks) {
            gl::Acc160 acc;
            acc.clear();
            u64 ref = 0;
            for (int i = 0; i < k; i++) {
                const u64 a = all_ones ? ~0ULL : rnd_word(), b = all_ones ? ~0ULL : rnd_word();
                acc.fma(a, b);
                ref = addmod(ref, mulmod(a % gl::P, b % gl::P));
            }
            const u64 got = acc.reduce();
            CHECK(got < gl::P, "Acc160: reduce() of %d terms is not canonical: %016llx", k, (unsigned long long)got);
            CHECK(got == ref, "Acc160: %d terms (all ones: %d): %016llx != %016llx", k, all_ones, (unsigned long long)got, (unsigned long long)ref);
        }
    // The documented bound, "at most 2^32 terms": the state after 2^32 - 1 products of 2^64 - 1 by itself, written down in
    // closed form, takes the last one.  M = (2^64 - 1)^2 = 2^128 - 2^65 + 1;  (2^32 - 1) M as five 32-bit words.
    const u64 K = (u64)1 << 32;
    const u64 m_lo = 1, m_hi = ~0ULL - 1;                       // M = m_hi 2^64 + m_lo
    const u128 lo = (u128)m_lo * (K - 1), hi = (u128)m_hi * (K - 1) + (u64)(lo >> 64);
    gl::Acc160 acc;
    acc.w[0] = (u32)lo;
    acc.w[1] = (u32)(lo >> 32);
    acc.w[2] = (u32)hi;
    acc.w[3] = (u32)(hi >> 32);
    acc.w[4] = (u32)(hi >> 64);
    CHECK((hi >> 96) == 0, "the closed form does not fit 160 bits");
    acc.fma(~0ULL, ~0ULL);
    CHECK(acc.w[4] == 0xFFFFFFFFu, "Acc160: top word after 2^32 all-ones terms is %08x", acc.w[4]);   // 2^32 M = 2^160 - 2^97 + 2^32
    const u64 m_mod = mulmod(~0ULL % gl::P, ~0ULL % gl::P);
    const u64 got = acc.reduce();
    CHECK(got < gl::P && got == mulmod(K % gl::P, m_mod), "Acc160: 2^32 all-ones terms: %016llx", (unsigned long long)got);
}

static void check_acc160x2() {
    for (int k : {1, 2, 5, 118}) {
        gl::Acc160x2 pair;
        gl::Acc160 s0, s1;
        pair.clear();
        s0.clear();
        s1.clear();
        for (int i = 0; i < k; i++) {
            const u64 term = rnd_word(), alpha[2] = {rnd_word(), rnd_word()};
            pair.fma_base(term, alpha);
            s0.fma(term, alpha[0]);
            s1.fma(term, alpha[1]);
        }
        for (int i = 0; i < 5; i++) CHECK(pair.s0.w[i] == s0.w[i] && pair.s1.w[i] == s1.w[i], "Acc160x2::fma_base: word %d after %d terms", i, k);
        const gl::e2 r = pair.reduce();
        CHECK(r.c0 == s0.reduce() && r.c1 == s1.reduce(), "Acc160x2::reduce after %d terms", k);
    }
    const u64 edges[] = {0, 1, gl::P - 1};
    std::vector<gl::e2> alphas;
    for (u64 a0 : edges)
        for (u64 a1 : edges) alphas.push_back({a0, a1});
    for (int i = 0; i < 100; i++) alphas.push_back({rnd_canon(), rnd_canon()});
    gl::Acc160x2 pair;
    pair.clear();
    gl::e2 ref{0, 0};
    for (size_t i = 0; i < alphas.size(); i++)
        for (int zero_c1 = 0; zero_c1 < 2; zero_c1++) {
            const gl::e2 t{i % 7 == 0 ? gl::P - 1 : rnd_canon(), zero_c1 ? 0 : rnd_canon()};
            gl::Acc160x2 one;
            one.clear();
            one.fma_e2(t, alphas[i].c0, alphas[i].c1);
            const gl::e2 prod = gl::e2_mul(t, alphas[i]), got = one.reduce();
            CHECK(got.c0 == prod.c0 && got.c1 == prod.c1, "Acc160x2::fma_e2: one term, alpha %zu", i);
            pair.fma_e2(t, alphas[i].c0, alphas[i].c1);
            ref = gl::e2_add(ref, prod);
            const gl::e2 sum = pair.reduce();
            CHECK(sum.c0 == ref.c0 && sum.c1 == ref.c1, "Acc160x2::fma_e2: running sum at alpha %zu", i);
        }
}

static void check_inversion() {
    std::vector<u64> xs = {0, 1, 2, 7, gl::P - 1, gl::P - 2, 0xFFFFFFFFULL, 0x100000000ULL};
    const size_t n_special = xs.size();
    for (int i = 0; i < 1000; i++) xs.push_back(rnd_canon());
    CHECK(gl::inv_chain(0) == 0, "inv_chain(0) = %016llx", (unsigned long long)gl::inv_chain(0));
    for (u64 x : xs) {
        const u64 got = gl::inv_chain(x);
        CHECK(got == gl::inv(x), "inv_chain(%016llx) = %016llx", (unsigned long long)x, (unsigned long long)got);
        if (x) CHECK(mulmod(got, x) == 1, "inv_chain(%016llx) is no inverse", (unsigned long long)x);
    }
    auto same = [](gl::e2 a) {
        const gl::e2 got = gl::e2_inv_chain(a), want = gl::e2_inv(a);
        CHECK(got.c0 == want.c0 && got.c1 == want.c1, "e2_inv_chain(%016llx, %016llx)", (unsigned long long)a.c0, (unsigned long long)a.c1);
    };
    for (size_t i = 0; i < n_special; i++)
        for (size_t j = 0; j < n_special; j++) same({xs[i], xs[j]});
    for (size_t i = n_special; i < xs.size(); i++) {
        same({xs[i], xs[xs.size() - 1 - (i - n_special)]});
        same({xs[i], xs[i % n_special]});
        same({xs[i % n_special], xs[i]});
    }
}

static void check_mul7_pow7() {
    std::vector<u64> as = {0, 1, gl::P - 1, gl::P / 7 - 1, gl::P / 7, gl::P / 7 + 1};
    for (int i = 0; i < 1000; i++) as.push_back(rnd_canon());
    for (u64 a : as) {
        CHECK(gl::mul7(a) == gl::mul(a, 7) && gl::mul7(a) == mulmod(a, 7), "mul7(%016llx)", (unsigned long long)a);
        CHECK(gl::pow7(a) == gl::pow(a, 7), "pow7(%016llx)", (unsigned long long)a);
    }
}

static void check_twiddle_table_readers() {
    for (unsigned log_n = 0; log_n <= 6; log_n++) {
        const u32 n = 1u << log_n;
        const u64 w = gl::omega(log_n);
        // T[j] = omega_n^bitrev(j, log_n - 1), j < n/2, on the heap at its exact size (one entry, omega^0, for n = 1)
        std::vector<u64> table(n / 2 ? n / 2 : 1);
        for (u32 j = 0; j < table.size(); j++) table[j] = gl::pow(w, log_n ? gl::bitrev32(j, log_n - 1) : 0);
        const u64 *tw = table.data();
        for (u32 r = 0; r < n; r++) {
            const u64 got = gl::omega_pow_nat(log_n ? tw : nullptr, log_n, r);   // n = 1 reads no table
            CHECK(got == gl::pow(w, r), "omega_pow_nat(log_n %u, r %u) = %016llx", log_n, r, (unsigned long long)got);
        }
        for (u32 j = 0; j < n; j++) {
            const u64 got = gl::domain_point(tw, j);
            CHECK(got == gl::pow(w, gl::bitrev32(j, log_n)), "domain_point(log_n %u, j %u) = %016llx", log_n, j, (unsigned long long)got);
        }
    }
}

int main() {
    check_acc160();
    check_acc160x2();
    check_inversion();
    check_mul7_pow7();
    check_twiddle_table_readers();
    check_reduce128_grid();
    printf("gl toolbox == 128-bit arithmetic (%d checks)\n", checks);
    return 0;
}
