// icikt_hclust.hip -- agglomerative clustering of the samples under raw with complete, average or single linkage, run on
// the device as S - 1 dependent steps over an S x S table of keys (icikt_hclust_f64, host side: icikt_capi_hclust.cpp).
//
// The rule.
//   SIMILARITY   of two samples: the pair's raw as its colsort::cor_key (order-preserving, -0 equal to +0).  A pair with
//                a reason code or an NA raw has no similarity: NA_KEY.
//   CLUSTERS     a cluster lives in the slot of its smallest sample; slot i starts as sample i.  Slots a < b merge
//                into a.
//   NA           the similarity of the merged cluster to any other live cluster k is NA if either old similarity is NA:
//                two clusters are mergeable exactly when every sample pair across them has a raw.
//   UPDATE       of the similarities w_a, w_b of a and b to k, both values: "complete" the smaller key, "single" the
//                larger key, "average" (n_a w_a + n_b w_b) / (n_a + n_b) on the decoded doubles, re-encoded; the sizes
//                n_a, n_b are exact doubles and the expression is __dmul_rn, __dmul_rn, __dadd_rn, __dadd_rn, __ddiv_rn
//                in this order, without contraction: five correctly rounded IEEE operations.
//   ORDER        each step merges the best live pair of clusters in a STRICT ORDER: the larger similarity first, then
//                the smaller a, then the smaller b.  The order is total, so the result is a pure function of the input,
//                whatever the block cut or the launch geometry.
//   END          merging stops at the first step whose best similarity is NA or, with min_raw (NaN: no bound), below
//                min_raw.  What is left is a forest; its components are numbered by their smallest sample.
//   VALUES       a merge's raw is its key decoded (so -0 is +0); its cor is raw / max(taumax) over all pairs with
//                scale_max (k_assemble's expression), else raw.
//
// The kernels.  k_hc_expand writes the symmetric table W [S][S] from the kept triangle (launch_median_keep's plane) with
// NA_KEY on the diagonal, and alive[s] = 1, size[s] = 1.  k_hc_rescan over all rows then gives every row s its best
// live partner in the strict order, nn[s] with nnkey[s] (-1 and key 0 -- which cor_key gives for no double -- for
// none): seen from one row the order is "the larger key, then the smaller partner", because a partner below s makes
// the pair's a smaller than any partner above s does.  A step is three launches on the stream, no host wait between:
//   k_hc_pick    one workgroup: the best (nnkey[i], min(i, nn[i]), max(i, nn[i])) over live i.  It writes merge record
//                t, sets alive[b] = 0 and size[a] += size[b], zeroes the rescan counter and publishes a, b, n_a, n_b;
//                without a candidate that passes it sets `done`, and every later launch of the call returns at once.
//   k_hc_merge   one thread per slot k: for live k outside {a, b} the updated similarity goes to W[a][k] and W[k][a].
//                If nn[k] was a or b, k goes on the rescan list (one atomic on the counter); else (k, a) becomes k's
//                neighbour if it is strictly better in the order -- equal keys can move a neighbour from c to a < c.
//                a itself always goes on the list.
//   k_hc_rescan  a fixed grid: workgroup g takes list entries g, g + G, .. and recomputes the row's neighbour.
// Why a row off the list keeps a valid cache: for all three methods the updated similarity is never above both old
// ones, and (k, c) was at least as good as (k, a) and (k, b); so (k, a) can only tie with it, which the merge kernel
// checks.  Nothing here waits on another workgroup; the only atomic is the list counter's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {

namespace {

using namespace colsort;

// first pair of row i of combn(S, 2) (cut_rows' formula, icikt_blocks.h)
__device__ __forceinline__ long long hc_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

// the double a key that is not NA_KEY stands for (cor_key's inverse; -0 was stored as +0)
__device__ __forceinline__ double hc_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// the better of two partners of one row: the larger key, equal keys by the smaller partner.  key 0: none
__device__ __forceinline__ void hc_better_partner(unsigned long long& key, int& t, unsigned long long k2, int t2) {
  if (k2 > key || (k2 == key && t2 < t)) { key = k2; t = t2; }
}

// the better of two pairs a < b in the strict order.  key 0: none
__device__ __forceinline__ void hc_better_pair(unsigned long long& key, int& a, int& b, unsigned long long k2, int a2,
                                               int b2) {
  if (k2 > key || (k2 == key && (a2 < a || (a2 == a && b2 < b)))) { key = k2; a = a2; b = b2; }
}

// the updated similarity of the merged cluster to k
__device__ __forceinline__ unsigned long long hc_update(int method, unsigned long long wa, unsigned long long wb,
                                                        double na, double nb) {
#pragma clang fp contract(off)
  if (wa == NA_KEY || wb == NA_KEY) return NA_KEY;
  if (method == HCLUST_COMPLETE) return wa < wb ? wa : wb;
  if (method == HCLUST_SINGLE) return wa > wb ? wa : wb;
  // __dmul_rn, __dmul_rn, __dadd_rn, __dadd_rn, __ddiv_rn.  The toolchain's header defines these as the plain operators
  // under ITS contraction setting, which an inlined call keeps (a product and a sum of theirs fuse into v_fmac_f64):
  // the operators are written out under this function's contract(off) instead, and the ISA holds two v_mul_f64, two
  // v_add_f64 and the division's expansion.
  const double sa = na * hc_value(wa);
  const double sb = nb * hc_value(wb);
  const double num = sa + sb;
  const double den = na + nb;
  return cor_key(num / den);
}

// grid (ceil(S / CT), S): cell (i = blockIdx.y, j) of the table from the triangle; row 0's workgroups also set the flags
__global__ void __launch_bounds__(CT)
k_hc_expand(const unsigned long long* __restrict__ kept, int S, unsigned long long* __restrict__ W,
            int32_t* __restrict__ alive, int32_t* __restrict__ size) {
  const int i = (int)blockIdx.y;
  const int j = (int)(blockIdx.x * CT + threadIdx.x);
  if (i >= S || j >= S) return;
  unsigned long long k = NA_KEY;
  if (i != j) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    k = kept[hc_rowoff(S, lo) + (hi - lo - 1)];
  }
  W[(long long)i * S + j] = k;
  if (i == 0) { alive[j] = 1; size[j] = 1; }
}

// Workgroup g recomputes the neighbour of rows list[g], list[g + G], .. below the list's count (all != 0: of rows g,
// g + G, .. below S): the best live partner of the row, read contiguously.
__global__ void __launch_bounds__(CT)
k_hc_rescan(const unsigned long long* __restrict__ W, const int32_t* __restrict__ alive, const int32_t* __restrict__ list,
            const int32_t* __restrict__ state, int S, int all, int32_t* __restrict__ nn,
            unsigned long long* __restrict__ nnkey) {
  __shared__ unsigned long long s_key[CT / 64];
  __shared__ int s_t[CT / 64];
  if (state[HC_DONE]) return;                          // (the same for every thread of the grid)
  const int tid = threadIdx.x;
  int count = all ? S : state[HC_COUNT];
  if (count > S) count = S;
  for (int e = (int)blockIdx.x; e < count; e += (int)gridDim.x) {
    const int w = all ? e : list[e];
    if (w < 0 || w >= S) continue;                     // (uniform; the merge kernel lists slots below S only)
    const unsigned long long* row = W + (long long)w * S;
    unsigned long long key = 0ull;
    int bt = 0x7FFFFFFF;
    for (int j = tid; j < S; j += CT) {
      if (j == w || !alive[j]) continue;
      const unsigned long long k = row[j];
      if (k == NA_KEY) continue;
      hc_better_partner(key, bt, k, j);
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long k2 = __shfl_xor(key, o, 64);
      const int t2 = __shfl_xor(bt, o, 64);
      hc_better_partner(key, bt, k2, t2);
    }
    if ((tid & 63) == 0) { s_key[tid >> 6] = key; s_t[tid >> 6] = bt; }
    __syncthreads();
    if (tid == 0) {
      for (int v = 1; v < CT / 64; ++v) hc_better_partner(key, bt, s_key[v], s_t[v]);
      nn[w] = key ? bt : -1;
      nnkey[w] = key;
    }
    __syncthreads();                                   // the slots are free for the next entry
  }
}

// One workgroup: the best pair over the live rows' neighbours; thread 0 records the merge or ends the call.
__global__ void __launch_bounds__(CT)
k_hc_pick(const int32_t* __restrict__ nn, const unsigned long long* __restrict__ nnkey, int32_t* alive, int32_t* size,
          int32_t* state, HcMerge* __restrict__ rec, unsigned long long min_key, int S) {
  __shared__ unsigned long long s_key[CT / 64];
  __shared__ int s_a[CT / 64], s_b[CT / 64];
  if (state[HC_DONE]) return;
  const int tid = threadIdx.x;
  unsigned long long key = 0ull;
  int a = 0x7FFFFFFF, b = 0x7FFFFFFF;
  for (int i = tid; i < S; i += CT) {
    if (!alive[i]) continue;
    const unsigned long long k = nnkey[i];
    const int t = nn[i];
    if (k == 0ull || k == NA_KEY || t < 0 || t >= S || t == i) continue;
    hc_better_pair(key, a, b, k, i < t ? i : t, i < t ? t : i);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k2 = __shfl_xor(key, o, 64);
    const int a2 = __shfl_xor(a, o, 64);
    const int b2 = __shfl_xor(b, o, 64);
    hc_better_pair(key, a, b, k2, a2, b2);
  }
  if ((tid & 63) == 0) { s_key[tid >> 6] = key; s_a[tid >> 6] = a; s_b[tid >> 6] = b; }
  __syncthreads();                                     // (every read of state and alive above lies before it)
  if (tid != 0) return;
  for (int v = 1; v < CT / 64; ++v) hc_better_pair(key, a, b, s_key[v], s_a[v], s_b[v]);
  const int t = state[HC_MERGES];
  if (key == 0ull || key < min_key || t < 0 || t >= S - 1 || !alive[a] || !alive[b]) {
    state[HC_DONE] = 1;
    return;
  }
  const int na = size[a], nb = size[b];
  rec[t].a = a;
  rec[t].b = b;
  rec[t].key = key;
  rec[t].size = na + nb;
  rec[t].pad = 0;
  alive[b] = 0;
  size[a] = na + nb;
  state[HC_MERGES] = t + 1;
  state[HC_COUNT] = 0;
  state[HC_A] = a;
  state[HC_B] = b;
  state[HC_NA] = na;
  state[HC_NB] = nb;
}

// One thread per slot k.  Thread k reads W[a][k] and W[b][k] and writes W[a][k] and W[k][a]: no thread reads what
// another writes.
__global__ void __launch_bounds__(CT)
k_hc_merge(unsigned long long* W, int32_t* nn, unsigned long long* nnkey, const int32_t* __restrict__ alive,
           int32_t* __restrict__ list, int32_t* state, int method, int S) {
  if (state[HC_DONE]) return;
  const int k = (int)(blockIdx.x * CT + threadIdx.x);
  if (k >= S) return;
  const int a = state[HC_A], b = state[HC_B];
  if (a < 0 || b < 0 || a >= S || b >= S) return;      // (pick publishes slots below S only)
  if (k == a) {
    const int at = atomicAdd(&state[HC_COUNT], 1);
    if (at < S) list[at] = a;
    return;
  }
  if (k == b || !alive[k]) return;
  const unsigned long long w = hc_update(method, W[(long long)a * S + k], W[(long long)b * S + k], (double)state[HC_NA],
                                         (double)state[HC_NB]);
  W[(long long)a * S + k] = w;
  W[(long long)k * S + a] = w;
  const int t = nn[k];
  if (t == a || t == b) {
    const int at = atomicAdd(&state[HC_COUNT], 1);
    if (at < S) list[at] = k;
  } else if (w != NA_KEY) {
    const unsigned long long cur = nnkey[k];
    if (w > cur || (w == cur && a < t)) { nn[k] = a; nnkey[k] = w; }
  }
}

}  // namespace

hipError_t launch_hc_expand(const unsigned long long* kept, int S, unsigned long long* W, int32_t* alive, int32_t* size,
                            hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (S > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_hc_expand, dim3((unsigned)((S + colsort::CT - 1) / colsort::CT), (unsigned)S), dim3(colsort::CT), 0,
                     s, kept, S, W, alive, size);
  return hipGetLastError();
}

hipError_t launch_hc_rescan(const unsigned long long* W, const int32_t* alive, const int32_t* list, const int32_t* state,
                            int S, int all, int grid, int32_t* nn, unsigned long long* nnkey, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (S > 65535 || grid < 1 || grid > HCLUST_GRID_MAX) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_hc_rescan, dim3((unsigned)grid), dim3(colsort::CT), 0, s, W, alive, list, state, S, all, nn, nnkey);
  return hipGetLastError();
}

hipError_t launch_hc_pick(const int32_t* nn, const unsigned long long* nnkey, int32_t* alive, int32_t* size,
                          int32_t* state, HcMerge* rec, unsigned long long min_key, int S, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (S > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_hc_pick, dim3(1), dim3(colsort::CT), 0, s, nn, nnkey, alive, size, state, rec, min_key, S);
  return hipGetLastError();
}

hipError_t launch_hc_merge(unsigned long long* W, int32_t* nn, unsigned long long* nnkey, const int32_t* alive,
                           int32_t* list, int32_t* state, int method, int S, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (S > 65535 || method < HCLUST_COMPLETE || method > HCLUST_SINGLE) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_hc_merge, dim3((unsigned)((S + colsort::CT - 1) / colsort::CT)), dim3(colsort::CT), 0, s, W, nn,
                     nnkey, alive, list, state, method, S);
  return hipGetLastError();
}

}  // namespace icikt
