// icikt_mst.hip -- the maximum spanning forest of the samples under raw, found on the device by Boruvka rounds over the
// kept plane (icikt_mst_f64, host side: icikt_capi_mst.cpp).
//
// The rule.  A pair i < j is a CANDIDATE EDGE iff its raw is not NA (reason code 0) and, when min_raw is given, raw >=
// min_raw as a plain IEEE comparison (icikt_edge_rule's; a NaN bound is no bound).  STRICT EDGE ORDER: the larger raw
// first, compared through colsort::cor_key (so -0 equals +0), equal keys broken by the smaller combn index (i
// ascending, then j ascending).  The order is total, so the maximum spanning forest under it is unique: a pure
// function of the input, whatever the block cut, the round structure or the launch geometry.
//
// The pair engine runs the whole combn triangle in blocks of rows; after each block k_median_keep (icikt_medians.hip)
// writes every pair's raw as an order-preserving 64-bit key (NA_KEY for a pair with a reason code) into the kept plane,
// in combn order.  After the last block the host runs Boruvka rounds: k_mst_best finds, for every sample, the best edge
// in the strict order that leaves the sample's component; the host picks each component's best among its members'
// candidates, merges by union-find and uploads the new components (O(S) per round, at most MST_MAX_ROUNDS rounds).
// Nothing here waits on another workgroup or issues a global atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {

namespace {

using namespace colsort;

// first pair of row i of combn(S, 2) (cut_rows' formula, icikt_blocks.h)
__device__ __forceinline__ long long mst_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

// the better of two candidates in the strict order, seen from one sample: the larger key, equal keys by the smaller
// partner (for a fixed s the combn index of {s, t} increases with t).  key 0 is no valid key (cor_key gives it for no
// double): "none" loses against every candidate.
__device__ __forceinline__ void mst_better(unsigned long long& key, int& t, unsigned long long k2, int t2) {
  if (k2 > key || (k2 == key && t2 < t)) { key = k2; t = t2; }
}

// One workgroup per sample s = blockIdx.x.  Among the partners t != s of another component whose key is a value
// (not NA_KEY) of at least min_key, the best in the strict order goes to best[s]; key 0, t -1 when there is none.
// t > s: row s of the triangle, contiguous in t; t < s: column s of row t, strided (k_class_select's addressing).
// live[s] == 0: the sample's component found nothing in an earlier round, and finds nothing now.
__global__ void __launch_bounds__(CT)
k_mst_best(const unsigned long long* __restrict__ kept, const int32_t* __restrict__ comp, const int32_t* __restrict__ live,
           unsigned long long min_key, int S, MstBest* __restrict__ best) {
  __shared__ unsigned long long s_key[CT / 64];
  __shared__ int s_t[CT / 64];
  const int tid = threadIdx.x;
  const int s = (int)blockIdx.x;
  if (s >= S) return;                                 // (the same for every thread of the workgroup)
  if (!live[s]) {
    if (tid == 0) { best[s].key = 0ull; best[s].t = -1; best[s].pad = 0; }
    return;
  }
  const int cs = comp[s];
  const long long row_s = mst_rowoff(S, s) - s - 1;   // + t: the pair (s, t), t > s
  unsigned long long key = 0ull;
  int bt = 0x7FFFFFFF;
  for (int t = tid; t < S; t += CT) {                 // ascending t per thread: a later equal key never wins
    if (t == s || comp[t] == cs) continue;
    const unsigned long long k = t > s ? kept[row_s + t] : kept[mst_rowoff(S, t) + (s - t - 1)];
    if (k == NA_KEY || k < min_key) continue;
    mst_better(key, bt, k, t);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k2 = __shfl_xor(key, o, 64);
    const int t2 = __shfl_xor(bt, o, 64);
    mst_better(key, bt, k2, t2);
  }
  if ((tid & 63) == 0) { s_key[tid >> 6] = key; s_t[tid >> 6] = bt; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < CT / 64; ++w) mst_better(key, bt, s_key[w], s_t[w]);
  best[s].key = key;
  best[s].t = key ? bt : -1;
  best[s].pad = 0;
}

}  // namespace

hipError_t launch_mst_best(const unsigned long long* kept, const int32_t* comp, const int32_t* live,
                           unsigned long long min_key, int S, MstBest* best, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (S > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mst_best, dim3((unsigned)S), dim3(colsort::CT), 0, s, kept, comp, live, min_key, S, best);
  return hipGetLastError();
}

}  // namespace icikt
