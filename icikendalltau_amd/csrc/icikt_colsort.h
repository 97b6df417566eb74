// icikt_colsort.h -- the per-column sort of the column pre-passes: cor_fast's (k_cor_prep, icikt_cor.hip) and the
// missing-value diagnostics' (k_diag_col, icikt_diag.hip).  One workgroup of CT threads per column: order-preserving
// 64-bit keys (missing last), a bitonic sort of the keys with their rows in the workgroup's global scratch, and the
// tie groups of the sorted keys.  Device code only; included by the .hip sources.
#ifndef ICIKT_COLSORT_H
#define ICIKT_COLSORT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icikt {
namespace colsort {

constexpr int CT = 256;                // threads of the per-column and per-pair workgroups
constexpr int SORT_TILE = 2048;        // bitonic stages with a distance below this run in LDS
constexpr uint64_t NA_KEY = ~0ull;

__device__ inline uint64_t cor_key(double v) {   // order-preserving, NaN last, -0 == +0
  if (v != v) return NA_KEY;
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// inclusive scan over the workgroup (CT threads, 4 waves); sh: 4 slots
template <typename T, typename Op>
__device__ inline T block_scan(T v, T* sh, Op op, T ident) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, u);
  }
  if (lane == 63) sh[w] = v;
  __syncthreads();
  T pre = ident;
  for (int k = 0; k < w; ++k) pre = op(pre, sh[k]);
  __syncthreads();
  return op(pre, v);
}

template <typename T, typename Op>
__device__ inline T block_reduce(T v, T* sh, Op op) {
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = op(op(sh[0], sh[1]), op(sh[2], sh[3]));
  __syncthreads();
  return v;
}


// ctr[idx] += 1 for every lane of the wave with idx >= 0, runs of equal idx in neighbouring lanes as ONE atomic of the
// run's length: the top digits of the keys and the bins of tied data are the same for most of a wave, and LDS atomics
// on one address serialise.  Every lane of the wave must call it.
__device__ __forceinline__ void run_add(unsigned int* ctr, int idx) {
  const int lane = (int)(threadIdx.x & 63u);
  const int prev = __shfl_up(idx, 1, 64);
  const bool head = lane == 0 || idx != prev;
  const unsigned long long heads = __ballot(head);
  if (head && idx >= 0) {
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = after ? __ffsll((long long)after) : 64 - lane;   // lanes up to the next run's head
    atomicAdd(&ctr[idx], (unsigned int)len);
  }
}

struct Add { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Max { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct Min { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };

__device__ inline bool bitonic_swap(uint64_t a, uint64_t b, bool up) { return up ? (a > b) : (a < b); }

// ascending bitonic sort of np2 (a power of two) keys with their rows, in this workgroup's global scratch; stages of
// distance < SORT_TILE run in LDS tile by tile
__device__ void block_sort(uint64_t* keys, int32_t* idx, int np2, uint64_t* sk, int32_t* si) {
  const int tile = np2 < SORT_TILE ? np2 : SORT_TILE;
  // merge sizes k_first .. k_last, their stages of distance < tile, tile by tile in LDS
  auto run_tiles = [&](int k_first, int k_last) {
    for (int t0 = 0; t0 < np2; t0 += tile) {
      for (int t = threadIdx.x; t < tile; t += CT) { sk[t] = keys[t0 + t]; si[t] = idx[t0 + t]; }
      __syncthreads();
      for (int k = k_first; k <= k_last; k <<= 1)
        for (int j = (k >> 1) < (tile >> 1) ? (k >> 1) : (tile >> 1); j > 0; j >>= 1) {
          for (int t = threadIdx.x; t < tile / 2; t += CT) {
            const int i = 2 * j * (t / j) + (t % j), l = i + j;
            const uint64_t a = sk[i], b = sk[l];
            if (bitonic_swap(a, b, ((t0 + i) & k) == 0)) {
              sk[i] = b; sk[l] = a;
              const int32_t x = si[i]; si[i] = si[l]; si[l] = x;
            }
          }
          __syncthreads();
        }
      for (int t = threadIdx.x; t < tile; t += CT) { keys[t0 + t] = sk[t]; idx[t0 + t] = si[t]; }
      __syncthreads();
    }
  };
  run_tiles(2, tile);
  for (int k = 2 * tile; k <= np2; k <<= 1) {
    for (int j = k >> 1; j >= tile; j >>= 1) {
      for (int t = threadIdx.x; t < np2 / 2; t += CT) {
        const int i = 2 * j * (t / j) + (t % j), l = i + j;
        const uint64_t a = keys[i], b = keys[l];
        if (bitonic_swap(a, b, (i & k) == 0)) {
          keys[i] = b; keys[l] = a;
          const int32_t x = idx[i]; idx[i] = idx[l]; idx[l] = x;
        }
      }
      __syncthreads();   // (orders the workgroup's global accesses)
    }
    run_tiles(k, k);
  }
}

// Tie groups of the sorted keys[0, cnt): f(p, g0, g1) for every position p, once, with [g0, g1) the positions of its
// group (equal keys).  gs: cnt ints of global scratch (holds each position's g0 afterwards); sh: 4 ints of LDS.
// Every thread of the workgroup calls it.
template <typename F>
__device__ inline void tie_groups(const uint64_t* keys, int cnt, int32_t* gs, int* sh, F f) {
  // group starts: running max of the positions that start a group
  int carry = 0;
  for (int b = 0; b < cnt; b += CT) {
    const int p = b + threadIdx.x;
    int v = 0;
    if (p < cnt) v = (p == 0 || keys[p] != keys[p - 1]) ? p : 0;
    v = block_scan(v, sh, Max(), 0);
    v = v > carry ? v : carry;
    if (p < cnt) gs[p] = v;
    if (threadIdx.x == CT - 1) sh[0] = v;
    __syncthreads();
    carry = sh[0];
    __syncthreads();
  }
  // group ends: running min from the right
  carry = cnt;
  for (int b = 0; b < cnt; b += CT) {
    const int p = cnt - 1 - (b + threadIdx.x);   // reversed positions
    int v = cnt;
    if (p >= 0) v = (p == cnt - 1 || keys[p] != keys[p + 1]) ? p + 1 : cnt;
    v = block_scan(v, sh, Min(), cnt);
    v = v < carry ? v : carry;
    if (p >= 0) f(p, (int)gs[p], v);
    if (threadIdx.x == CT - 1) sh[0] = v;
    __syncthreads();
    carry = sh[0];
    __syncthreads();
  }
}

}  // namespace colsort
}  // namespace icikt
#endif
