// icikt_select.h -- the median of a workgroup's keys by a most-significant-digit radix select, as a function template
// over the key loader: the body k_median_select (icikt_medians.hip) states inline, shared by the kernels written after
// it (k_class_select, icikt_classmat.hip).  One workgroup of colsort::CT threads calls it together; the keys are
// colsort::cor_key values, NA_KEY for a key that is no value.  Device code only; included by the .hip sources.
#ifndef ICIKT_SELECT_H
#define ICIKT_SELECT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icikt_colsort.h"

namespace icikt {
namespace sel {

constexpr uint64_t R_NA_BITS = 0x7FF00000000007A2ull;    // R's NA_real_
constexpr uint64_t R_NAN_BITS = 0x7FF8000000000000ull;   // R_NaN

// the LDS a select needs besides the caller's staging buffer: 1 084 B
struct Scratch {
  unsigned int hist[256];
  int red[4];
  unsigned long long red64[4];
  int pick[3];   // digit, rank inside the digit's bin, keys of the bin
};

__device__ inline double key_value(uint64_t k) {   // inverse of cor_key (a zero comes back as +0)
  const uint64_t b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}
// R's mean() of the middle two: the correctly rounded midpoint; 0.5 (a + b) unless a + b overflows
__device__ inline double mean2(double a, double b) {
  const double s = a + b;
  if (s - s == 0.0) return 0.5 * s;
  if (a - a == 0.0 && b - b == 0.0) return 0.5 * a + 0.5 * b;   // finite values whose sum overflows
  return s != s ? __longlong_as_double((long long)R_NAN_BITS) : s;
}
__device__ inline double plus_zero(double v) { return v == 0.0 ? 0.0 : v; }

// The two middle keys of the T keys key_at(0 .. T - 1).  Returns v, the keys below NA_KEY, to every thread; with v > 0
// *lower is the key of rank (v - 1) >> 1 among the valid keys ascending and *upper the key of rank v >> 1 (the same
// key when v is odd).  key_at is called 9 to 10 times per key: from LDS when the caller has staged the keys, else it
// re-reads them.  Every thread of the workgroup calls this, after a barrier behind the caller's staging stores.
template <typename KeyAt>
__device__ inline int middle_keys(int T, KeyAt key_at, Scratch& sh, unsigned long long* lower, unsigned long long* upper) {
  using namespace colsort;
  const int tid = threadIdx.x;
  int cnt = 0;
  for (int q = tid; q < T; q += CT) cnt += key_at(q) != NA_KEY;
  const int v = block_reduce(cnt, sh.red, Add());
  if (v == 0) return 0;
  // the key of rank k among the T keys (NA_KEY is above every valid key, and k < v): digit by digit from the top
  int k = (v - 1) >> 1, bin = 0;
  unsigned long long prefix = 0ull, mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    sh.hist[tid] = 0u;
    __syncthreads();
    for (int q = tid; q < T; q += CT) {
      const unsigned long long key = key_at(q);
      if ((key & mask) == prefix) atomicAdd(&sh.hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const int h = (int)sh.hist[tid];
    const int incl = block_scan(h, sh.red, Add(), 0);
    if (incl - h <= k && k < incl) { sh.pick[0] = tid; sh.pick[1] = k - (incl - h); sh.pick[2] = h; }
    __syncthreads();
    prefix |= (unsigned long long)sh.pick[0] << shift;
    mask |= 0xFFull << shift;
    k = sh.pick[1];
    bin = sh.pick[2];
    __syncthreads();
  }
  // prefix: the lower middle key, k: its rank inside its run of `bin` equal keys.  An even count takes the next rank
  // too: the same key while the run covers it, else the smallest key above
  unsigned long long up = prefix;
  if (!(v & 1) && k + 1 >= bin) {
    unsigned long long lo = NA_KEY;
    for (int q = tid; q < T; q += CT) {
      const unsigned long long key = key_at(q);
      if (key > prefix && key < lo) lo = key;
    }
    up = block_reduce(lo, sh.red64, Min());
  }
  *lower = prefix;
  *upper = up;
  return v;
}

// The medians of raw and of cor from the middle keys of v > 0 values.  rk: word 0 of launch_out_stats' record, the
// largest taumax as a key (0: no pair had one).  The division is k_assemble's, on k_assemble's operands.
__device__ inline void median_values(unsigned long long lower, unsigned long long upper, int v, unsigned long long rk,
                                     int scale_max, double* med_cor, double* med_raw) {
  const double a = key_value(lower), b = key_value(upper);
  // max(numeric(0), na.rm = TRUE) is -Inf in R
  const double max_cor = rk ? __longlong_as_double((long long)((rk >> 63) ? (rk & 0x7FFFFFFFFFFFFFFFull) : ~rk))
                            : -__longlong_as_double(0x7FF0000000000000ll);
  const double ca = scale_max ? plus_zero(a / max_cor) : a, cb = scale_max ? plus_zero(b / max_cor) : b;
  *med_raw = (v & 1) ? a : plus_zero(mean2(a, b));
  *med_cor = (v & 1) ? ca : plus_zero(mean2(ca, cb));
}

}  // namespace sel
}  // namespace icikt
#endif
