// Internal: the challenges of the lookup argument as its two kernels (stage2.hip, quotient.hip) take them.
#pragma once
#include "gl.h"
#include "term_io.h"

namespace bj {
// beta and gamma^0 .. gamma^w; A: a kernel's argument struct {gl::e2 beta; gl::e2 gpow[9];}
template <class A>
inline A lookup_challenges(const LookupArg &l) {
    A a;
    a.beta = {gl::canon(l.h_beta[0]), gl::canon(l.h_beta[1])};
    const gl::e2 g{gl::canon(l.h_gamma[0]), gl::canon(l.h_gamma[1])};
    a.gpow[0] = {1, 0};
    for (unsigned j = 1; j <= l.w && j < 9; j++) a.gpow[j] = gl::e2_mul(a.gpow[j - 1], g);
    return a;
}
}  // namespace bj
