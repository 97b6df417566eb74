// icikt_classmat.hip -- every sample's median ICI-Kendall-tau to every class, reduced on the device
// (icikt_class_matrix_f64, host side: icikt_capi_classmat.cpp).
//
// The pair engine runs the whole combn triangle in blocks of rows; after each block k_median_keep (icikt_medians.hip)
// writes every pair's raw as an order-preserving 64-bit key (NA_KEY for a pair with a reason code) into the kept plane,
// in combn order.  After the last block k_class_select runs one workgroup per (sample, class) cell: the cell's keys are
// the sample's pairs with the class's members, gathered through the member list, and the median is found by the radix
// select of icikt_select.h.  Nothing here waits on another workgroup or issues a global atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_select.h"

namespace icikt {

namespace {

using namespace colsort;

// first pair of row i of combn(S, 2) (cut_rows' formula, icikt_blocks.h)
__device__ __forceinline__ long long cm_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

// One workgroup per cell (s, c) = (blockIdx.x, blockIdx.y).  Class c is member[first[c] .. first[c + 1]); key q of the
// cell belongs to t = member[first[c] + q]: NA_KEY for the sample itself, else the pair (min, max) of the triangle --
// t > s: row s, contiguous in t; t < s: column s of row t, strided.  stage: keys the LDS buffer takes
// (<= MEDIAN_STAGE_MAX); a cell with more keys re-reads the member list and the kept plane in every pass.
__global__ void __launch_bounds__(CT)
k_class_select(const int32_t* __restrict__ member, const int32_t* __restrict__ first,
               const unsigned long long* __restrict__ kept, const unsigned long long* __restrict__ red, int S, int n_class,
               int scale_max, int stage, double* __restrict__ med2, int32_t* __restrict__ n_valid) {
  __shared__ unsigned long long s_keys[MEDIAN_STAGE_MAX];
  __shared__ sel::Scratch s_sel;
  const int tid = threadIdx.x;
  const int s = (int)blockIdx.x, c = (int)blockIdx.y;
  if (s >= S || c >= n_class) return;
  const int f0 = first[c];
  const int T = first[c + 1] - f0;
  const long long row_s = cm_rowoff(S, s) - s - 1;   // + t: the pair (s, t), t > s
  const bool staged = T <= stage;
  auto load = [&](int q) -> unsigned long long {
    const int t = member[f0 + q];
    if (t == s) return NA_KEY;
    return t > s ? kept[row_s + t] : kept[cm_rowoff(S, t) + (s - t - 1)];
  };
  if (staged)
    for (int q = tid; q < T; q += CT) s_keys[q] = load(q);
  __syncthreads();
  auto key_at = [&](int q) -> unsigned long long { return staged ? s_keys[q] : load(q); };

  unsigned long long lower = 0ull, upper = 0ull;
  const int v = sel::middle_keys(T, key_at, s_sel, &lower, &upper);
  if (tid != 0) return;
  const size_t cell = (size_t)c * (size_t)S + (size_t)s, plane = (size_t)S * (size_t)n_class;
  if (v == 0) {   // no partner: an empty class, the sample's own singleton class, or NA pairs alone
    med2[cell] = __longlong_as_double((long long)sel::R_NA_BITS);
    med2[plane + cell] = __longlong_as_double((long long)sel::R_NA_BITS);
    n_valid[cell] = 0;
    return;
  }
  double med_cor, med_raw;
  sel::median_values(lower, upper, v, red[0], scale_max, &med_cor, &med_raw);
  med2[cell] = med_cor;
  med2[plane + cell] = med_raw;
  n_valid[cell] = v;
}

}  // namespace

hipError_t launch_class_select(const int32_t* member, const int32_t* first, const unsigned long long* kept,
                               const unsigned long long* red, int S, int n_class, int scale_max, int stage, double* med2,
                               int32_t* n_valid, hipStream_t s) {
  if (S <= 0 || n_class <= 0) return hipSuccess;
  if (stage < 0 || stage > MEDIAN_STAGE_MAX || n_class > CLASS_MATRIX_MAX_CLASSES) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_class_select, dim3((unsigned)S, (unsigned)n_class), dim3(colsort::CT), 0, s, member, first, kept,
                     red, S, n_class, scale_max, stage, med2, n_valid);
  return hipGetLastError();
}

}  // namespace icikt
