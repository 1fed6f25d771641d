// Stand-alone host program for tests/test_w16_shift_host.py: the host fallbacks of csrc/gl.h's butterflies by 16th roots of unity.
// Reads pairs "u v" (hex) from stdin; for every pair prints, for the forward and the inverse root and every exponent e = 0..7, the
// canonical results of w16_butterfly_weak<e> and of both halves of w16_butterfly2_weak on the step's pairs; then for every shift S the
// canonical mul_pow2_weak<S>(v).  It also checks each against 128-bit arithmetic itself, so that a sanitizer build finds what the
// comparison in Python could not.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gl.h"

using gl::u64;
typedef unsigned __int128 u128;
static int failures = 0;
static u64 mulmod(u64 a, u64 b) { return (u64)((u128)a * b % gl::P); }
static void expect(u64 got, u64 want, const char *what, int e, u64 u, u64 v) {
    if (gl::canon(got) != want && failures++ < 10) fprintf(stderr, "%s e/S=%d u=%llx v=%llx: %llx != %llx\n", what, e, (unsigned long long)u, (unsigned long long)v, (unsigned long long)gl::canon(got), (unsigned long long)want);
}
template <int E, bool INV>
static void one(u64 u, u64 v) {
    const u64 w = gl::cx_pow(gl::cx_pow(0x185629dcda58878cULL, 1ULL << 28), INV ? (16 - E) % 16 : E);
    static_assert(gl::w16<E, INV>::S % 12 == 0 && gl::w16<E, INV>::S < 96, "a 16th root is a power of 2^12");
    const u64 t = mulmod(v % gl::P, w), s = (u64)(((u128)(u % gl::P) + t) % gl::P), d = (u64)(((u128)(u % gl::P) + gl::P - t) % gl::P);
    u64 a = u, b = v;
    gl::w16_butterfly_weak<E, INV>(a, b);
    expect(a, s, "sum", E, u, v);
    expect(b, d, "difference", E, u, v);
    printf(" %llx %llx", (unsigned long long)gl::canon(a), (unsigned long long)gl::canon(b));
}
template <int EA, int EB, bool INV>
static void two(u64 u, u64 v) {
    u64 ua = u, va = v, ub = u, vb = v, xa = u, ya = v, xb = u, yb = v;
    gl::w16_butterfly2_weak<EA, EB, INV>(ua, va, ub, vb);
    gl::w16_butterfly_weak<EA, INV>(xa, ya);
    gl::w16_butterfly_weak<EB, INV>(xb, yb);
    expect(ua, gl::canon(xa), "pair a sum", EA, u, v);
    expect(va, gl::canon(ya), "pair a difference", EA, u, v);
    expect(ub, gl::canon(xb), "pair b sum", EB, u, v);
    expect(vb, gl::canon(yb), "pair b difference", EB, u, v);
}
template <bool INV>
static void direction(u64 u, u64 v) {
    one<0, INV>(u, v); one<1, INV>(u, v); one<2, INV>(u, v); one<3, INV>(u, v);
    one<4, INV>(u, v); one<5, INV>(u, v); one<6, INV>(u, v); one<7, INV>(u, v);
    two<0, 4, INV>(u, v); two<2, 6, INV>(u, v); two<1, 5, INV>(u, v); two<3, 7, INV>(u, v); two<4, 4, INV>(u, v); two<0, 0, INV>(u, v);
}
template <int S>
static void shift(u64 v) {
    const u64 r = gl::mul_pow2_weak<S>(v);
    expect(r, mulmod(v % gl::P, gl::cx_pow(2, S)), "mul_pow2_weak", S, 0, v);
    printf(" %llx", (unsigned long long)gl::canon(r));
}

int main() {
    std::vector<u64> in;
    unsigned long long x;
    while (scanf("%llx", &x) == 1) in.push_back(x);
    if (in.size() % 2) return 2;
    for (size_t i = 0; i < in.size(); i += 2) {
        const u64 u = in[i], v = in[i + 1];
        direction<false>(u, v);
        direction<true>(u, v);
        shift<12>(v); shift<24>(v); shift<36>(v); shift<48>(v); shift<60>(v); shift<72>(v); shift<84>(v);
        printf("\n");
    }
    if (failures) {
        fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    fprintf(stderr, "w16 butterflies == 128-bit arithmetic on %zu pairs\n", in.size() / 2);
    return 0;
}
