// icikt_medians.hip -- per-sample median ICI-Kendall-tau within classes, reduced on the device (icikt_class_medians_f64,
// host side: icikt_capi_medians.cpp).
//
// The pair engine runs the within-class pairs in blocks; after each block k_median_keep writes every pair's raw as an
// order-preserving 64-bit key (colsort::cor_key; NA_KEY for a pair with a reason code) into the kept plane, at the
// pair's place in the call's pair order: class by class, combn order inside a class.  After the last block
// k_median_select runs one workgroup per sample: the sample's partners are one strided and one contiguous run of its
// class's triangle in the kept plane, and the order statistic (v - 1) >> 1 of the v valid keys is found by a
// most-significant-digit radix select (8-bit digits, 256 LDS counters), not by a sort: few rows give a few hundred
// distinct taus among thousands of partners.  Nothing here waits on another workgroup or issues a global atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {

namespace {

using namespace colsort;

constexpr uint64_t R_NA_BITS = 0x7FF00000000007A2ull;    // R's NA_real_
constexpr uint64_t R_NAN_BITS = 0x7FF8000000000000ull;   // R_NaN

// (sorted_median's rule and key_value of icikt_diag.hip, on the one or two middle values instead of a sorted array:
//  moving them to a shared header would have to leave every existing kernel's code identical, so the few lines are
//  stated again)
__device__ inline double md_key_value(uint64_t k) {   // inverse of cor_key (a zero comes back as +0)
  const uint64_t b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}
// R's mean() of the middle two: the correctly rounded midpoint; 0.5 (a + b) unless a + b overflows
__device__ inline double md_mean2(double a, double b) {
  const double s = a + b;
  if (s - s == 0.0) return 0.5 * s;
  if (a - a == 0.0 && b - b == 0.0) return 0.5 * a + 0.5 * b;   // finite values whose sum overflows
  return s != s ? __longlong_as_double((long long)R_NAN_BITS) : s;
}
__device__ inline double md_plus_zero(double v) { return v == 0.0 ? 0.0 : v; }

// first pair of row i of combn(m, 2) (cut_rows' formula, icikt_host.h)
__device__ __forceinline__ long long md_rowoff(long long m, long long i) { return i * (2 * m - i - 1) / 2; }

__global__ void __launch_bounds__(256)
k_median_keep(const double* __restrict__ out4, const int32_t* __restrict__ reasons, long long n_pairs,
              unsigned long long* __restrict__ kept) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_pairs) return;
  kept[e] = reasons[e] != 0 ? NA_KEY : cor_key(out4[4 * e]);
}

// One workgroup per sample s: position r among the m members of its class, whose first pair is pair `base` of the kept
// plane.  Partner q of the m - 1: q < r the member a = q (pair (a, r): base + rowoff(m, a) + r - a - 1, strided), else
// the member b = q + 1 (pair (r, b): base + rowoff(m, r) + q - r, contiguous).  stage: keys the LDS buffer takes
// (<= MEDIAN_STAGE_MAX); a sample with more partners re-reads the kept plane in every pass.
__global__ void __launch_bounds__(CT)
k_median_select(MedianClasses mc, const unsigned long long* __restrict__ kept, const unsigned long long* __restrict__ red,
                int S, int scale_max, int stage, double* __restrict__ med2, int32_t* __restrict__ n_valid) {
  __shared__ unsigned long long s_keys[MEDIAN_STAGE_MAX];
  __shared__ unsigned int s_hist[256];
  __shared__ int s_red[4];
  __shared__ unsigned long long s_red64[4];
  __shared__ int s_pick[3];   // digit, rank inside the digit's bin, keys of the bin
  const int tid = threadIdx.x;
  const int s = (int)blockIdx.x;
  if (s >= S) return;
  const int m = mc.size[s], r = mc.pos[s];
  const long long base = mc.base[s];
  const int T = m - 1;
  const long long row_r = base + md_rowoff(m, r) - r;   // + q: the contiguous run
  const bool staged = T <= stage;
  auto load = [&](int q) -> unsigned long long {
    return q < r ? kept[base + md_rowoff(m, q) + (r - q - 1)] : kept[row_r + q];
  };
  if (staged)
    for (int q = tid; q < T; q += CT) s_keys[q] = load(q);
  __syncthreads();
  auto key_at = [&](int q) -> unsigned long long { return staged ? s_keys[q] : load(q); };

  int cnt = 0;
  for (int q = tid; q < T; q += CT) cnt += key_at(q) != NA_KEY;
  const int v = block_reduce(cnt, s_red, Add());
  if (v == 0) {   // no partner (a singleton class, or NA pairs alone)
    if (tid == 0) {
      med2[s] = __longlong_as_double((long long)R_NA_BITS);
      med2[(size_t)S + s] = __longlong_as_double((long long)R_NA_BITS);
      n_valid[s] = 0;
    }
    return;
  }
  // the key of rank k among the T keys (NA_KEY is above every valid key, and k < v): digit by digit from the top
  int k = (v - 1) >> 1, bin = 0;
  unsigned long long prefix = 0ull, mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    s_hist[tid] = 0u;
    __syncthreads();
    for (int q = tid; q < T; q += CT) {
      const unsigned long long key = key_at(q);
      if ((key & mask) == prefix) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const int h = (int)s_hist[tid];
    const int incl = block_scan(h, s_red, Add(), 0);
    if (incl - h <= k && k < incl) { s_pick[0] = tid; s_pick[1] = k - (incl - h); s_pick[2] = h; }
    __syncthreads();
    prefix |= (unsigned long long)s_pick[0] << shift;
    mask |= 0xFFull << shift;
    k = s_pick[1];
    bin = s_pick[2];
    __syncthreads();
  }
  // prefix: the lower middle key, k: its rank inside its run of `bin` equal keys.  An even count takes the next rank
  // too: the same key while the run covers it, else the smallest key above
  unsigned long long upper = prefix;
  if (!(v & 1) && k + 1 >= bin) {
    unsigned long long lo = NA_KEY;
    for (int q = tid; q < T; q += CT) {
      const unsigned long long key = key_at(q);
      if (key > prefix && key < lo) lo = key;
    }
    upper = block_reduce(lo, s_red64, Min());
  }
  if (tid == 0) {
    const double a = md_key_value(prefix), b = md_key_value(upper);
    // max(numeric(0), na.rm = TRUE) is -Inf in R; the division is k_assemble's, on k_assemble's operands
    const unsigned long long rk = red[0];
    const double max_cor = rk ? __longlong_as_double((long long)((rk >> 63) ? (rk & 0x7FFFFFFFFFFFFFFFull) : ~rk))
                              : -__longlong_as_double(0x7FF0000000000000ll);
    const double ca = scale_max ? md_plus_zero(a / max_cor) : a, cb = scale_max ? md_plus_zero(b / max_cor) : b;
    med2[(size_t)S + s] = (v & 1) ? a : md_plus_zero(md_mean2(a, b));
    med2[s] = (v & 1) ? ca : md_plus_zero(md_mean2(ca, cb));
    n_valid[s] = v;
  }
}

}  // namespace

hipError_t launch_median_keep(const double* out4, const int32_t* reasons, long long n_pairs, unsigned long long* kept,
                              hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_median_keep, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, out4, reasons, n_pairs, kept);
  return hipGetLastError();
}

hipError_t launch_median_select(const MedianClasses& mc, const unsigned long long* kept, const unsigned long long* red,
                                int S, int scale_max, int stage, double* med2, int32_t* n_valid, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (stage < 0 || stage > MEDIAN_STAGE_MAX) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_median_select, dim3((unsigned)S), dim3(colsort::CT), 0, s, mc, kept, red, S, scale_max, stage, med2,
                     n_valid);
  return hipGetLastError();
}

}  // namespace icikt
