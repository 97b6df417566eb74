// icikt_mantel.h -- the arithmetic of the Mantel test (icikt_mantel_*: DESIGN.md section 28) that is no device code: the
// two quantisations, the limb split of a product and the comparison of two sums.  Plain C++ for the host and the device,
// no device header: tests/test_mantel_host.py compiles it alone (tests/mantel_print.cpp), icikt_mantel.hip calls it in
// its quantisation kernels, icikt_capi_mantel.cpp in its comparison, and api._mantel_numpy and tests/mantel_checker.py
// restate it.
//
// THE RULE (method = pearson).  raw is the double of the pair's kept key (cor_key's inverse: -0 has become +0).
//   xv = llrint(ldexp(1.0 - raw, 30))           one subtraction, an exact scaling, one rounding half to even: raw is a
//                                               correlation in [-1, 1], so xv is in 0 .. 2^31
//   yv = llrint(ldexp(y - lo, 31 - e))          lo and hi the smallest and largest y, span = hi - lo one double
//                                               operation, (m, e) = frexp(span): span = m 2^e with m in [0.5, 1), so
//                                               y - lo <= span < 2^e and yv is in 0 .. 2^31.  A span of 0 (a constant y)
//                                               has e = 0 and every yv = 0; a span that is not finite is refused
// The scalings are exact and the subtractions stand alone: there is nothing an fma could be contracted from, and the
// pragma below says so to the compiler that would.  Both values move by at most 2^-31 of their range.
// method = spearman needs no arithmetic here: both vectors are doubled average ranks, integers in 2 .. 2 P < 2^32.
//
// THE LIMBS.  A product xv yv is below 2^64; its low 32 bits and the rest are summed apart, each in 64 bits, and
// T = hi 2^32 + lo.  With at most P < 2^31 products either sum stays below 2^63.  Two T are compared as 128-bit integers
// (T < 2^95).
#ifndef ICIKT_MANTEL_H
#define ICIKT_MANTEL_H

#include <cmath>

#if defined(__HIP__)   // (compiled as HIP: the attributes are the compiler's own)
#define ICIKT_MANTEL_FN __host__ __device__ inline
#else
#define ICIKT_MANTEL_FN inline
#endif

namespace icikt {
namespace mantel {

constexpr int X_FRAC_BITS = 30;                     // xv = (1 - raw) 2^30
constexpr int Y_BITS = 31;                          // yv = (y - lo) 2^(31 - e)
constexpr unsigned long long V_MAX = 1ull << 31;    // the largest xv or yv of method pearson
constexpr int METHOD_PEARSON = 0, METHOD_SPEARMAN = 1;

// the double of a key that is neither 0 nor NA_KEY (host::cor_key_value; a zero comes back as +0)
ICIKT_MANTEL_FN double key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}

// xv of a raw value that is not NaN
ICIKT_MANTEL_FN unsigned long long quantise_x(double raw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = 1.0 - raw;
  return (unsigned long long)::llrint(::ldexp(d, X_FRAC_BITS));
}

// the exponent e of span = hi - lo: (m, e) = frexp(span); 0 for a span of 0
ICIKT_MANTEL_FN int span_exponent(double span) {
  int e = 0;
  (void)::frexp(span, &e);
  return e;
}

// yv of a finite y >= lo, e = span_exponent(hi - lo)
ICIKT_MANTEL_FN unsigned long long quantise_y(double y, double lo, int e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = y - lo;
  return (unsigned long long)::llrint(::ldexp(d, Y_BITS - e));
}

// a value's two limbs: v = hi 2^32 + lo
ICIKT_MANTEL_FN unsigned long long limb_lo(unsigned long long v) { return v & 0xFFFFFFFFull; }
ICIKT_MANTEL_FN unsigned long long limb_hi(unsigned long long v) { return v >> 32; }

// -1, 0, 1 as hi_a 2^32 + lo_a is below, equal to, above hi_b 2^32 + lo_b (limb sums, each below 2^63)
ICIKT_MANTEL_FN int compare_sums(unsigned long long lo_a, unsigned long long hi_a, unsigned long long lo_b,
                                 unsigned long long hi_b) {
  const unsigned __int128 a = ((unsigned __int128)hi_a << 32) + lo_a, b = ((unsigned __int128)hi_b << 32) + lo_b;
  return a < b ? -1 : (a > b ? 1 : 0);
}

}  // namespace mantel
}  // namespace icikt
#endif
