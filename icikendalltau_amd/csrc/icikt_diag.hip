// icikt_diag.hip -- the missing-value diagnostics of the reference (R/left_censorship.R, R/rank-ordering.R):
// calculate_matrix_medians, test_left_censorship's per-class counts and rank_order_data's ranks and medians.
//
//   KD0  k_diag_col          one workgroup per column: the global_na rule, missing / excluded counts, the sort of the
//                            non-missing values (icikt_colsort.h, shared with cor_fast), the median (or NA); rank mode:
//                            each cell's doubled rank(x, na.last = FALSE) as an int32
//   KD1  k_diag_censor       one thread per row, walking each class's columns: trials, successes and missing cells of
//                            the rows with a missing cell; one 64-bit atomic per workgroup, class and count
//        k_diag_rowmiss      one thread per row of a class: its missing count, kept flag, and the kept rows' count
//        k_diag_median_rank  one thread per kept row: the median of its n_cols doubled ranks by a 4-bit radix select
//                            (counters in LDS), no per-row sort
//   KD2  k_diag_gather       original / ordered: the kept rows of the class's columns, in a given row and column order,
//                            bitwise copies, masked cells as NA_real_
// DESIGN.md section 10 restates the formulas and what bounds each kernel.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {
namespace {

using namespace colsort;

constexpr uint64_t R_NA_BITS = 0x7FF00000000007A2ull;    // R's NA_real_
constexpr uint64_t R_NAN_BITS = 0x7FF8000000000000ull;   // R_NaN

__device__ inline double key_value(uint64_t k) {   // inverse of cor_key (a zero comes back as +0)
  const uint64_t b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ inline bool cell_missing(const MaskSpec& ms, double v) { return v != v || mask_excluded(ms, v); }

// R's median of the sorted values s[0, m): the middle one, or mean() of the middle two (long double in R: the
// correctly rounded midpoint; 0.5 (a + b) unless a + b overflows, mean(c(-Inf, Inf)) = NaN)
__device__ inline double sorted_median(const uint64_t* keys, int m) {
  if (m & 1) return key_value(keys[m >> 1]);
  const double a = key_value(keys[(m >> 1) - 1]), b = key_value(keys[m >> 1]);
  const double s = a + b;
  if (s - s == 0.0) return 0.5 * s;
  if (a - a == 0.0 && b - b == 0.0) return 0.5 * a + 0.5 * b;   // finite values whose sum overflows
  return s != s ? __longlong_as_double((long long)R_NAN_BITS) : s;
}

__global__ void __launch_bounds__(CT) k_diag_col(DiagCol dc) {
  __shared__ int shi[4];
  __shared__ uint64_t sk[SORT_TILE];
  __shared__ int32_t si[SORT_TILE];
  const int64_t n = dc.n;
  uint64_t* keys = dc.keys + (int64_t)blockIdx.x * dc.np2;
  int32_t* idx = dc.idx + (int64_t)blockIdx.x * dc.np2;
  int32_t* gs = dc.gs + (int64_t)blockIdx.x * dc.np2;
  for (int c = blockIdx.x; c < dc.S; c += gridDim.x) {
    const double* x = dc.X + (int64_t)c * dc.ld;
    int cnt = 0, nex = 0, kmiss = 0;
    for (int r = threadIdx.x; r < dc.np2; r += CT) {
      uint64_t key = NA_KEY;
      if (r < n) {
        const double v = x[r];
        const bool ex = mask_excluded(dc.ms, v), miss = ex || v != v;
        nex += ex;
        cnt += !miss;
        if (dc.rank2 && miss && dc.kept[r]) ++kmiss;
        if (!miss) key = cor_key(v);
      }
      keys[r] = key;
      idx[r] = r < n ? r : -1;
    }
    cnt = block_reduce(cnt, shi, Add());
    nex = block_reduce(nex, shi, Add());
    kmiss = block_reduce(kmiss, shi, Add());
    block_sort(keys, idx, dc.np2, sk, si);
    if (threadIdx.x == 0) {
      const int nmiss = (int)n - cnt;
      const bool na = cnt == 0 || (nmiss > 0 && !dc.na_rm);
      dc.median[c] = na ? __longlong_as_double((long long)R_NA_BITS) : sorted_median(keys, cnt);
      dc.nmiss[c] = nmiss;
      dc.nexcl[c] = nex;
    }
    if (dc.rank2) {
      // rank(x, na.last = FALSE) doubled: the kept rows' missing cells take 1 .. kmiss in row order, a value kmiss plus
      // its average rank among the values (a group at positions [g0, g1) averages (g0 + 1 + g1) / 2)
      int32_t* rk = dc.rank2 + (int64_t)c * n;
      tie_groups(keys, cnt, gs, shi, [&](int p, int g0, int g1) { rk[idx[p]] = 2 * kmiss + g0 + g1 + 1; });
      int carry = 0;
      for (int64_t b = 0; b < n; b += CT) {
        const int64_t r = b + threadIdx.x;
        bool miss = false, kept = false;
        if (r < n) {
          miss = cell_missing(dc.ms, x[r]);
          kept = dc.kept[r] != 0;
        }
        const int f = (miss && kept) ? 1 : 0;
        const int incl = block_scan(f, shi, Add(), 0) + carry;
        if (miss) rk[r] = kept ? 2 * incl : 0;   // dropped rows: no rank
        if (threadIdx.x == CT - 1) shi[0] = incl;
        __syncthreads();
        carry = shi[0];
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

// trials / successes / missing cells per class (the columns of class k: cols[off[k] .. off[k + 1]))
__global__ void __launch_bounds__(CT) k_diag_censor(const double* __restrict__ X, int64_t ld, int64_t n, MaskSpec ms,
                                                    const int32_t* __restrict__ cols, const int32_t* __restrict__ off,
                                                    int n_class, const double* __restrict__ median,
                                                    unsigned long long* __restrict__ out3) {
  __shared__ long long shl[4];
  const int64_t r = (int64_t)blockIdx.x * CT + threadIdx.x;
  for (int k = 0; k < n_class; ++k) {
    long long t = 0, s = 0, nm = 0;
    if (r < n) {
      for (int j = off[k]; j < off[k + 1]; ++j) {
        const int c = cols[j];
        const double v = X[(int64_t)c * ld + r], m = median[c];
        const bool miss = cell_missing(ms, v);
        nm += miss;
        if (!miss && m == m) {   // x < median is NA for a missing x and for an NA / NaN median
          ++t;
          s += v < m;
        }
      }
      if (nm == 0) t = s = 0;   // only rows with a missing cell are tested
    }
    t = block_reduce(t, shl, Add());
    s = block_reduce(s, shl, Add());
    nm = block_reduce(nm, shl, Add());
    if (threadIdx.x == 0) {
      if (t) atomicAdd(out3 + 3 * k, (unsigned long long)t);
      if (s) atomicAdd(out3 + 3 * k + 1, (unsigned long long)s);
      if (nm) atomicAdd(out3 + 3 * k + 2, (unsigned long long)nm);
    }
  }
}

// per row of a class's columns (n x n_cols, leading dimension n): missing cells, kept (not missing in every column)
__global__ void __launch_bounds__(CT) k_diag_rowmiss(const double* __restrict__ X, int64_t n, int n_cols, MaskSpec ms,
                                                     int32_t* __restrict__ n_na, uint8_t* __restrict__ kept,
                                                     unsigned long long* __restrict__ n_kept) {
  __shared__ long long shl[4];
  const int64_t r = (int64_t)blockIdx.x * CT + threadIdx.x;
  long long k = 0;
  if (r < n) {
    int m = 0;
    for (int j = 0; j < n_cols; ++j) m += cell_missing(ms, X[(int64_t)j * n + r]);
    n_na[r] = m;
    kept[r] = m < n_cols;
    k = m < n_cols;
  }
  k = block_reduce(k, shl, Add());
  if (threadIdx.x == 0 && k) atomicAdd(n_kept, (unsigned long long)k);
}

// median of a kept row's n_cols doubled ranks (integers below 2^20): the k-th smallest by five 4-bit digit passes over
// the row, each thread with 16 counters of its own in LDS; an even count takes one more pass for the next value
__global__ void __launch_bounds__(CT) k_diag_median_rank(const int32_t* __restrict__ rank2, int64_t n, int n_cols,
                                                         const uint8_t* __restrict__ kept, double* __restrict__ med) {
  __shared__ int ctr[16][CT];
  const int64_t r = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (r >= n) return;
  if (!kept[r]) {
    med[r] = __longlong_as_double((long long)R_NA_BITS);
    return;
  }
  const int t = threadIdx.x;
  int k = (n_cols - 1) >> 1;   // 0-based order statistic
  uint32_t prefix = 0;
  int eq = 0;
  for (int shift = 16; shift >= 0; shift -= 4) {
    for (int d = 0; d < 16; ++d) ctr[d][t] = 0;
    for (int j = 0; j < n_cols; ++j) {
      const uint32_t v = (uint32_t)rank2[(int64_t)j * n + r];
      if ((v >> (shift + 4)) == prefix) ++ctr[(v >> shift) & 15u][t];
    }
    int d = 0;
    while (k >= ctr[d][t]) { k -= ctr[d][t]; ++d; }
    eq = ctr[d][t];
    prefix = (prefix << 4) | (uint32_t)d;
  }
  const uint32_t v1 = prefix;
  if (n_cols & 1) {
    med[r] = 0.5 * (double)v1;
    return;
  }
  uint32_t v2 = v1;
  if (k + 1 >= eq) {   // the next order statistic is the smallest value above v1
    v2 = 0xFFFFFFFFu;
    for (int j = 0; j < n_cols; ++j) {
      const uint32_t v = (uint32_t)rank2[(int64_t)j * n + r];
      if (v > v1 && v < v2) v2 = v;
    }
  }
  med[r] = 0.25 * ((double)v1 + (double)v2);
}

// out[i + j n_out] = X[rows[i] + colsel[j] n], NA_real_ where the rule masks it
__global__ void __launch_bounds__(CT) k_diag_gather(const double* __restrict__ X, int64_t n, MaskSpec ms,
                                                    const int32_t* __restrict__ rows, int64_t n_out,
                                                    const int32_t* __restrict__ colsel, int n_cols,
                                                    double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (i >= n_out) return;
  for (int64_t j = blockIdx.y; j < n_cols; j += gridDim.y) {
    const uint64_t b = reinterpret_cast<const uint64_t*>(X)[(int64_t)colsel[j] * n + rows[i]];
    const bool miss = cell_missing(ms, __longlong_as_double((long long)b));
    reinterpret_cast<uint64_t*>(out)[j * n_out + i] = miss ? R_NA_BITS : b;
  }
}

}  // namespace

hipError_t launch_diag_col(const DiagCol& dc, int blocks, hipStream_t s) {
  if (dc.S <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_diag_col, dim3((unsigned)blocks), dim3(CT), 0, s, dc);
  return hipGetLastError();
}

hipError_t launch_diag_censor(const double* X, int64_t ld, int64_t n, const MaskSpec& ms, const int32_t* cols,
                              const int32_t* off, int n_class, const double* median, unsigned long long* out3,
                              hipStream_t s) {
  if (n <= 0 || n_class <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_diag_censor, dim3((unsigned)((n + CT - 1) / CT)), dim3(CT), 0, s, X, ld, n, ms, cols, off,
                     n_class, median, out3);
  return hipGetLastError();
}

hipError_t launch_diag_rowmiss(const double* X, int64_t n, int n_cols, const MaskSpec& ms, int32_t* n_na,
                               uint8_t* kept, unsigned long long* n_kept, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_diag_rowmiss, dim3((unsigned)((n + CT - 1) / CT)), dim3(CT), 0, s, X, n, n_cols, ms, n_na, kept,
                     n_kept);
  return hipGetLastError();
}

hipError_t launch_diag_median_rank(const int32_t* rank2, int64_t n, int n_cols, const uint8_t* kept, double* med,
                                   hipStream_t s) {
  if (n <= 0 || n_cols <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_diag_median_rank, dim3((unsigned)((n + CT - 1) / CT)), dim3(CT), 0, s, rank2, n, n_cols, kept,
                     med);
  return hipGetLastError();
}

hipError_t launch_diag_gather(const double* X, int64_t n, const MaskSpec& ms, const int32_t* rows, int64_t n_out,
                              const int32_t* colsel, int n_cols, double* out, hipStream_t s) {
  if (n_out <= 0 || n_cols <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_diag_gather, dim3((unsigned)((n_out + CT - 1) / CT), (unsigned)std::min(n_cols, 65535)), dim3(CT), 0,
                     s, X, n, ms, rows, n_out, colsel, n_cols, out);
  return hipGetLastError();
}

}  // namespace icikt
