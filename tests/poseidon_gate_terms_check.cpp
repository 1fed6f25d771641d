// Host check of csrc/poseidon_gate_terms.h: the two flattened Poseidon gate walks under the F_p^2 policy the verifier uses and
// under the canonical-u64 policy (host side) the quotient kernels use, against expected terms computed elsewhere.
// tests/test_poseidon_gate_terms_host.py draws the variables, evaluates the gates' op lists over F_p^2 with oracle/verifier.py
// (independent of the product), writes both to a file and builds this program for the host with the address and
// undefined-behaviour sanitizers.
//   file: for each gate (Poseidon2 first, then Poseidon v1): u64 count; count x { 130 x (c0, c1) variables, any u64 words;
//         118 x (c0, c1) expected terms, canonical }, little endian
// Every word of every term is compared; repetitions whose variables all have c1 = 0 also go through the u64 policy.
#include "poseidon_gate_terms.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using gl::e2;
using gl::u64;

constexpr unsigned N_VARS = 130, N_TERMS = 118;

template <class F, class Var>
static std::vector<typename F::elem> terms_of(int gate, Var var) {
    std::vector<typename F::elem> out;
    auto push = [&](typename F::elem t) { out.push_back(t); };
    if (gate == 0) bj::poseidon2_flattened_terms<F>(var, push);
    else bj::poseidon1_flattened_terms<F>(var, push);
    return out;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const char *names[2] = {"poseidon2", "poseidon1"};
    size_t words = 0, base_reps = 0;
    for (int gate = 0; gate < 2; gate++) {
        u64 count = 0;
        if (fread(&count, 8, 1, f) != 1 || count > 4096) return 2;
        for (u64 rep = 0; rep < count; rep++) {
            std::vector<u64> v(2 * N_VARS), want(2 * N_TERMS);
            if (fread(v.data(), 8, v.size(), f) != v.size() || fread(want.data(), 8, want.size(), f) != want.size()) return 2;
            const auto got = terms_of<bj::GateE2>(gate, [&](unsigned k) { return e2{gl::canon(v[2 * k]), gl::canon(v[2 * k + 1])}; });
            if (got.size() != N_TERMS) {
                printf("MISMATCH %s rep %llu: %zu terms\n", names[gate], (unsigned long long)rep, got.size());
                return 1;
            }
            bool base = true;
            for (unsigned k = 0; k < N_VARS; k++) base = base && gl::canon(v[2 * k + 1]) == 0;
            std::vector<u64> got64;
            if (base) {
                got64 = terms_of<bj::GateU64>(gate, [&](unsigned k) { return gl::canon(v[2 * k]); });
                base_reps++;
            }
            for (unsigned t = 0; t < N_TERMS; t++) {
                if (got[t].c0 != want[2 * t] || got[t].c1 != want[2 * t + 1] ||
                    (base && (got64.size() != N_TERMS || got64[t] != want[2 * t] || want[2 * t + 1] != 0))) {
                    printf("MISMATCH %s rep %llu term %u: e2 (%016llx, %016llx)%s want (%016llx, %016llx)\n", names[gate],
                           (unsigned long long)rep, t, (unsigned long long)got[t].c0, (unsigned long long)got[t].c1,
                           base ? " [u64 policy run too]" : "", (unsigned long long)want[2 * t], (unsigned long long)want[2 * t + 1]);
                    return 1;
                }
                words += base ? 3 : 2;
            }
        }
    }
    if (fgetc(f) != EOF) return 2;
    fclose(f);
    printf("poseidon gate walks == op lists over F_p^2: %zu words, %zu repetitions also under the u64 policy\n", words, base_reps);
    return 0;
}
