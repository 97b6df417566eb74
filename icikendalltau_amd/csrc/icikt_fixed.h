// icikt_fixed.h -- the fixed-point value a squared dissimilarity is summed as (icikt_permanova_*: DESIGN.md section 25).
// Plain C++ for the host and the device, no device header: tests/test_fixed_host.py compiles it alone
// (tests/fixed_print.cpp), icikt_permanova.hip calls it in its quantisation kernel, and api._permanova_numpy and
// tests/permanova_checker.py restate it.
//
// THE RULE.  raw is the double of the pair's kept key (cor_key's inverse: -0 has become +0).  d = 1.0 - raw and
// e = d * d are two IEEE double operations, each rounded once; q = llrint(ldexp(e, 50)) in the default rounding mode,
// round half to even.  raw is a correlation in [-1, 1], so d is in [0, 2], e in [0, 4] and q in 0 .. 2^52; the scaling
// by 2^50 is exact, and q 2^-50 is e itself (no rounding in this step) whenever e is a multiple of 2^-50; otherwise
// |q 2^-50 - e| <= 2^-51.  A subtraction and a product stand alone here: there is nothing an fma could be contracted
// from, and the pragma below says so to the compiler that would.
#ifndef ICIKT_FIXED_H
#define ICIKT_FIXED_H

#include <cmath>

#if defined(__HIP__)   // (compiled as HIP: the attributes are the compiler's own)
#define ICIKT_FIXED_FN __host__ __device__ inline
#else
#define ICIKT_FIXED_FN inline
#endif

namespace icikt {
namespace fixed {

constexpr int FRAC_BITS = 50;                        // q = e 2^50
constexpr unsigned long long Q_MAX = 1ull << 52;     // e <= 4
constexpr unsigned long long NA_KEY = ~0ull;         // colsort::NA_KEY, host::NA_KEY: a pair without a value

// the double of a key that is neither 0 nor NA_KEY (host::cor_key_value; a zero comes back as +0)
ICIKT_FIXED_FN double key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}

// q of a raw value that is not NaN
ICIKT_FIXED_FN unsigned long long quantise(double raw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = 1.0 - raw;
  const double e = d * d;
  return (unsigned long long)::llrint(::ldexp(e, FRAC_BITS));
}

// q of a kept key; NA_KEY (no value) adds nothing
ICIKT_FIXED_FN unsigned long long quantise_key(unsigned long long key) {
  return key == NA_KEY ? 0ull : quantise(key_value(key));
}

// a sum's two limbs: A = hi 2^32 + lo.  A sum of limbs of up to 2^31 values of at most 2^52 stays below 2^63 (lo) and
// 2^52 (hi)
ICIKT_FIXED_FN unsigned long long limb_lo(unsigned long long q) { return q & 0xFFFFFFFFull; }
ICIKT_FIXED_FN unsigned long long limb_hi(unsigned long long q) { return q >> 32; }

}  // namespace fixed
}  // namespace icikt
#endif
