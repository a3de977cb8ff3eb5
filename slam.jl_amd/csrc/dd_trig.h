// dd_trig.h -- sin and cos of a double as the CORRECTLY ROUNDED doubles, and a two-term dot product that loses nothing to
// cancellation (csrc/ekf_join.hip).
//
// Why: map joining turns a point p of the local map into a's frame with c = cos phi, s = sin phi and uses
// j0 = -(s px + c py), j1 = c px - s py as Jacobian entries.  Where the two products nearly cancel, one ulp of c or s (the gap
// between two libm implementations) or one rounding of a product is an error of u (|s px| + |c py|) in j, which can be many
// times u |j|: the result is then no longer within a few roundings of F P F' as the definition states it.  So c and s are
// the doubles nearest to the true cos and sin of the stored heading (what any careful evaluation agrees on), and the dot
// product is evaluated with its rounding errors carried (error about u |j| + u^2 (|s px| + |c py|)).
//
// sincos_rn: double-double arithmetic.  phi is reduced by k = rint(phi 2 / pi) quarter turns with pi / 2 as three doubles (good
// for |k| < 2^30; a stored heading is within a turn or two); sin r and cos r, |r| <= pi / 4 + 2^-50, are summed from their Taylor
// series in double-double, 16 terms each (the last one below 2^-120); the high word of the normalised sum is the rounded
// value.  One thread runs this once per join; it is not a fast path.  tests/test_join_ref_cpu.py compiles this header for the
// host (no contraction there: the device build's arithmetic is held by the per-entry bound of tests/test_gpu_ekf_join.py) and
// holds it to 60-digit decimal arithmetic and exact rationals over a sweep of angles.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DDT_FN __host__ __device__ inline
#else
#define DDT_FN inline
#endif

// The error-free transformations below are exact only as written: a compiler that contracts a product into the addition that
// follows it (clang's default for device code) feeds the sum a different value than the one whose error is then subtracted.
#if defined(__clang__)
#define DDT_EXACT _Pragma("clang fp contract(off)")
#else
#define DDT_EXACT
#endif

struct ddt { double h, l; };

DDT_FN ddt ddt_two_sum(double a, double b) {
    DDT_EXACT
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
DDT_FN ddt ddt_quick(double a, double b) {           // |a| >= |b|
    DDT_EXACT
    const double s = a + b;
    return {s, b - (s - a)};
}
DDT_FN ddt ddt_two_prod(double a, double b) {
    DDT_EXACT
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
DDT_FN ddt ddt_add(ddt a, ddt b) {
    DDT_EXACT
    ddt s = ddt_two_sum(a.h, b.h);
    const ddt t = ddt_two_sum(a.l, b.l);
    s.l += t.h;
    s = ddt_quick(s.h, s.l);
    s.l += t.l;
    return ddt_quick(s.h, s.l);
}
DDT_FN ddt ddt_mul(ddt a, ddt b) {
    DDT_EXACT
    ddt p = ddt_two_prod(a.h, b.h);
    p.l += a.h * b.l + a.l * b.h;
    return ddt_quick(p.h, p.l);
}
DDT_FN ddt ddt_div_d(ddt a, double b) {              // b: a small whole number here
    DDT_EXACT
    const double q1 = a.h / b;
    const ddt p = ddt_two_prod(q1, b);
    const double r = ((a.h - p.h) - p.l) + a.l;
    return ddt_quick(q1, r / b);
}
DDT_FN ddt ddt_neg(ddt a) { return {-a.h, -a.l}; }

// s = the double nearest to sin(phi), c = the double nearest to cos(phi)
DDT_FN void sincos_rn(double phi, double* s, double* c) {
    DDT_EXACT
    const double P1 = 1.5707963267948966, P2 = 6.123233995736766e-17, P3 = -1.4973849048591698e-33;      // pi / 2 = P1 + P2 + P3 + ...
    const double k = rint(phi * 0.63661977236758134);
    ddt r = ddt_add(ddt{phi, 0.0}, ddt_neg(ddt_two_prod(k, P1)));         // (phi - k P1 cancels exactly in the high words)
    r = ddt_add(r, ddt_neg(ddt_two_prod(k, P2)));
    r = ddt_add(r, ddt{-k * P3, 0.0});
    const ddt t = ddt_mul(r, r);
    ddt ss = r, ts = r, cs = {1.0, 0.0}, tc = {1.0, 0.0};
    for (int i = 1; i <= 16; ++i) {
        ts = ddt_neg(ddt_div_d(ddt_mul(ts, t), (double)((2 * i) * (2 * i + 1))));
        ss = ddt_add(ss, ts);
        tc = ddt_neg(ddt_div_d(ddt_mul(tc, t), (double)((2 * i - 1) * (2 * i))));
        cs = ddt_add(cs, tc);
    }
    const long long q = (long long)k & 3;
    *s = q == 0 ? ss.h : q == 1 ? cs.h : q == 2 ? -ss.h : -cs.h;
    *c = q == 0 ? cs.h : q == 1 ? -ss.h : q == 2 ? -cs.h : ss.h;
}

// a x + b y with the rounding errors of both products and of the sum carried along
DDT_FN double dot2_rn(double a, double x, double b, double y) {
    DDT_EXACT
    const ddt p = ddt_two_prod(a, x), q = ddt_two_prod(b, y), t = ddt_two_sum(p.h, q.h);
    return t.h + (t.l + (p.l + q.l));
}
