// icikt_keys.h -- the host's side of the two 64-bit encodings the device orders doubles by.  Plain C++, no device
// header: tests/test_keys_host.py compiles it alone (tests/keys_print.cpp).  The device states them where it uses them
// (colsort::cor_key in icikt_colsort.h, dbl_sortable in icikt_epilogue.hip; icikt_medians.hip says why they are
// restated there); the two differ in one value and are kept as two names:
//   the plain order   every double's bits made monotone, -0.0 below +0.0; 0 is below every double.  Word 0 of d_red
//                     (launch_out_stats: the largest taumax) and the top-k lists hold these
//   cor_key           the same bits after -0 has become +0, and NaN as NA_KEY, above every value.  The kept planes, the
//                     merge records and the spanning tree's edges hold these
#ifndef ICIKT_KEYS_H
#define ICIKT_KEYS_H

#include <cmath>
#include <cstring>

namespace icikt {
namespace host {

constexpr unsigned long long NA_KEY = ~0ull;                       // colsort::NA_KEY: a pair without a value
constexpr unsigned long long R_NA_BITS = 0x7FF00000000007A2ull;    // R's NA_real_

inline unsigned long long bits_of(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}
inline double from_bits(unsigned long long b) {
  double v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

// the double of a word of the plain order that is not 0 (dbl_unsortable)
inline double sortable_value(unsigned long long k) {
  return from_bits((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}
// word 0 of d_red as the largest taumax; 0: no pair had one, and max(numeric(0), na.rm = TRUE) is -Inf in R
inline double max_taumax_of(unsigned long long red0) { return red0 ? sortable_value(red0) : -HUGE_VAL; }

// colsort::cor_key: order-preserving, -0 stored as +0, NaN as NA_KEY
inline unsigned long long cor_key(double v) {
  if (v != v) return NA_KEY;
  if (v == 0.0) v = 0.0;
  const unsigned long long b = bits_of(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
// ... and back: the double of a key that is neither 0 nor NA_KEY (a zero comes back as +0)
inline double cor_key_value(unsigned long long k) {
  return from_bits((k >> 63) ? (k & ~(1ull << 63)) : ~k);
}

}  // namespace host
}  // namespace icikt
#endif
