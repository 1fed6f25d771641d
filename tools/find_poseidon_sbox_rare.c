/* S-box inputs x for which one product of x^7 takes the rare branches of gl::mul_weak (era_boojum_amd/csrc/gl.h): the final
 * subtraction borrows without the carry of the reduction multiply-add (class 1: the D - EPS correction applies) or with it
 * (class 3: the branch is entered and the s_andn2_b64 mask zeroes the correction).  The model of the instruction sequence is
 * tools/find_rare_mul_vectors.c's; every product is checked against 128-bit integers.  x^7 is taken in two chains:
 *   weak:      poseidon1.hip p1_pow7, mul_weak results passed on unreduced.  x is a residue >= 2^32 - 1, so its only u64
 *              representative is x itself and the device sees exactly that word whatever p1_add_rc did before;
 *   canonical: the flattened gates' pow7 (gate_poseidon.hip), gl::mul = canon(mul_weak) after every product.
 * Products: 0 = x*x, 1 = x2*x, 2 = x2*x2, 3 = x4*x3.  Class 1 comes from structured inputs (k * 2^48, 2^24, 2^14); class 3 from a
 * search (~2^-33 per product).  Class 1 at x2*x has no known construction: that cell stays empty.
 *   gcc -O3 -fopenmp tools/find_poseidon_sbox_rare.c -o /tmp/find_sbox && /tmp/find_sbox > tests/golden/poseidon_sbox_rare.json */
#include <stdint.h>
#include <stdio.h>
#include <omp.h>
typedef unsigned __int128 u128;
static const uint64_t P = 0xFFFFFFFF00000001ull, EPS = 0xFFFFFFFFull;
static const char *const CHAINS[2] = {"weak", "canonical"};
static const char *const PRODUCTS[4] = {"x*x", "x2*x", "x2*x2", "x4*x3"};
enum { WANT1 = 2, WANT3 = 1 };   /* entries per cell: class 3 costs ~2^33 candidates per hit */
static uint64_t splitmix(uint64_t *s) { uint64_t z = (*s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
/* the weak result of mul_weak; *cls: bit0 = borrow, bit1 = carry c (as find_rare_mul_vectors.c); with ok: *ok &= congruent
   to a * b (128-bit integers: slow, so the search runs without it and checks its hits) */
static uint64_t model(uint64_t a, uint64_t b, int *cls, int *ok) {
    uint32_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    uint64_t T = (uint64_t)a0 * b0;
    uint64_t U = (uint64_t)a0 * b1 + (T >> 32);
    u128 Xw = (u128)((uint64_t)a1 * b0) + U;
    uint64_t X = (uint64_t)Xw; int cm = (int)(Xw >> 64);
    uint64_t H = (uint64_t)a1 * b1 + (X >> 32);
    uint64_t lo = (uint32_t)T | (X << 32);
    u128 Rw = (u128)((uint64_t)(uint32_t)H * EPS) + lo;
    uint64_t R = (uint64_t)Rw; int c = (int)(Rw >> 64);
    uint64_t sub = (H >> 32) + (uint64_t)cm;
    int bo = R < sub;
    uint64_t D = R - sub;
    if (bo && !c) D -= EPS;
    uint64_t V = D + (c ? EPS : 0);
    *cls = bo | (c << 1);
    if (ok) *ok &= (V % P) == (uint64_t)(((u128)a * b) % P);
    return V;
}
static uint64_t canon(uint64_t v) { return v >= P ? v - P : v; }
/* classes of the four products of x^7 in one chain; with ok: *ok says whether every product was congruent */
static void pow7_classes(uint64_t x, int canonical, int cls[4], int *ok) {
    uint64_t x2 = model(x, x, &cls[0], ok);
    if (canonical) x2 = canon(x2);
    uint64_t x3 = model(x2, x, &cls[1], ok);
    uint64_t x4 = model(x2, x2, &cls[2], ok);
    if (canonical) x3 = canon(x3), x4 = canon(x4);
    model(x4, x3, &cls[3], ok);
}
static int found[2][4][4];
static int first = 1;
static void emit(int chain, int pos, int cls, uint64_t x) {
    printf("%s  {\"chain\": \"%s\", \"product\": \"%s\", \"position\": %d, \"class\": %d, \"x\": %llu}", first ? "" : ",\n", CHAINS[chain],
           PRODUCTS[pos], pos, cls, (unsigned long long)x);
    first = 0;
    fflush(stdout);
}
/* record every rare product of x that is still wanted; x must be a residue, and >= 2^32 - 1 for the weak chain */
static void offer(uint64_t x, int only_class) {
    for (int chain = 0; chain < 2; chain++) {
        if (chain == 0 && x < EPS) continue;
        int cls[4], ok = 1;
        pow7_classes(x, chain, cls, &ok);
        if (!ok) { fprintf(stderr, "model disagrees with integers at %llu\n", (unsigned long long)x); continue; }
        for (int pos = 0; pos < 4; pos++) {
            int k = cls[pos] & 3;
            if (!(k & 1) || (only_class && k != only_class)) continue;
#pragma omp critical
            if (found[chain][pos][k] < (k == 1 ? WANT1 : WANT3)) { found[chain][pos][k]++; emit(chain, pos, k, x); }
        }
    }
}
int main(void) {
    printf("{\n \"note\": \"S-box inputs x whose x^7 takes a rare branch of gl::mul_weak at the given product; chain weak = "
           "poseidon1.hip p1_pow7, canonical = the flattened gates' pow7; class 1 = borrow without carry (correction applied), "
           "3 = borrow with carry (branch entered, correction masked); found by tools/find_poseidon_sbox_rare.c\",\n \"entries\": [\n");
    /* class 1, structured: x * x = k^2 * 2^96 = -k^2 for x = k * 2^48; 2^24 and 2^14 reach 2^96 at x2 * x2 and x4 * x3 */
    const uint64_t seeds[] = {1ull << 48, 3ull << 48, 0xFFFFull << 48, 1ull << 24, 1ull << 14};
    for (unsigned i = 0; i < sizeof seeds / sizeof seeds[0]; i++) offer(seeds[i], 1);
    /* class 3, searched among residues >= 2^32 - 1 (valid in both chains) */
#pragma omp parallel
    {
        uint64_t seed = 0x5B0C5EEDull * (omp_get_thread_num() + 1);
        for (uint64_t it = 0;; it++) {
            if ((it & 0xFFFFF) == 0) {
                int left = 0;
#pragma omp critical
                for (int chain = 0; chain < 2; chain++)
                    for (int pos = 0; pos < 4; pos++) left += found[chain][pos][3] < WANT3;
                if (!left) break;
            }
            uint64_t x = splitmix(&seed);
            if (x >= P || x < EPS) continue;
            /* the integer check is slow: run the chains without it and offer x only when some product borrowed */
            int cls[4], hit = 0;
            for (int chain = 0; chain < 2 && !hit; chain++) {
                pow7_classes(x, chain, cls, NULL);
                for (int pos = 0; pos < 4; pos++) hit |= cls[pos] & 1;
            }
            if (hit) offer(x, 3);
        }
    }
    printf("\n ]\n}\n");
    return 0;
}
