// icikt_anosim.hip -- ANOSIM (Clarke 1993; vegan::anosim) of the samples' classes under the dissimilarity 1 - raw, with
// its permutation test, on the device (icikt_anosim_f64, host side: icikt_capi_anosim.cpp).
//
// The rule.  A pair i < j is a VALUE iff its raw is not NA (reason code 0: k_median_keep's rule); M is the number of
// values.  Values are ordered by colsort::cor_key(raw), so -0 equals +0 and equal doubles are equal keys.  A value's
// rank is its average rank among the M values in ascending dissimilarity 1 - raw, that is in DESCENDING raw, as R's
// rank(ties = "average") gives it; the device holds the DOUBLED rank r2 = 2 M - lo - hi + 1, lo the keys below the
// pair's key and hi the keys at or below it: an integer in 2 .. 2 M, and r2 = 0 marks a pair that is no value.  For a
// labelling L (a class index per sample) W2(L) is the sum of r2 over the values whose two samples share a class and
// nW(L) their count; the statistic R and its comparison between labellings are the host's, in integers
// (icikt_capi_anosim.cpp).  Everything here is an integer sum, a count or a comparison: the result is a pure function
// of the input and the labellings, whatever the block cut, the sort's tile, the strip, the batch or the grid.
//
// The pair engine runs the combn triangle in blocks of whole rows; after each block k_median_keep (icikt_medians.hip)
// writes the block's keys into the kept plane.  After the last block
//   k_anosim_count    one pass over the plane: M and the keys' digit table [8][256], so that the host skips the digits
//                     all keys share (the p.adjust fold's table, counted behind the keep instead of inside it: the keep
//                     stays the kernel four entries share, and the pass reads 8 bytes per pair once);
//   (the sort)        a copy of the plane sorted ascending by launch_padj_sort_pass (icikt_padjust.hip), NA keys last;
//   k_anosim_rank     one thread per pair: lo by a binary search in the first M sorted keys, hi by doubling steps from
//                     lo and a binary search in the bracket, r2 into the sort's free plane;
//   k_anosim_classes  the observed labelling's W2 and nW per class: one workgroup per row, one atomic pair per row;
//   k_anosim_perm     the hot path: W2 and nW of ANO_PB labellings at a time, see below.
// No kernel waits on another workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {

namespace {

using namespace colsort;

// ---- count: the valid keys and the digit table of the whole plane ------------------------------------------------

__global__ void __launch_bounds__(256)
k_anosim_count(const unsigned long long* __restrict__ kept, long long n, unsigned long long* __restrict__ total,
               unsigned long long* __restrict__ dhist) {
  __shared__ unsigned int s_hist[8 * 256];
  __shared__ unsigned int s_valid;
  const int tid = (int)threadIdx.x;
  for (int q = tid; q < 8 * 256; q += 256) s_hist[q] = 0u;
  if (tid == 0) s_valid = 0u;
  __syncthreads();
  unsigned int nv = 0u;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long e = base + tid;
    const bool in = e < n;
    const unsigned long long key = in ? kept[e] : NA_KEY;
    nv += (unsigned int)__popcll(__ballot(in && key != NA_KEY));
#pragma unroll
    for (int d = 0; d < 8; ++d) run_add(s_hist + d * 256, in ? (int)((key >> (8 * d)) & 255ull) : -1);
  }
  if ((tid & 63) == 0) atomicAdd(&s_valid, nv);   // the ballots gave every lane the wave's count
  __syncthreads();
  if (tid == 0 && s_valid) atomicAdd(total, (unsigned long long)s_valid);
  for (int q = tid; q < 8 * 256; q += 256) {
    const unsigned int c = s_hist[q];
    if (c) atomicAdd(&dhist[q], (unsigned long long)c);
  }
}

// ---- rank: the doubled average rank of every pair ------------------------------------------------------------------

// sorted[0, m): the values' keys ascending (the NA keys lie behind them).  r2[e] = 2 m - lo - hi + 1, 0 for an NA pair
__global__ void __launch_bounds__(256)
k_anosim_rank(const unsigned long long* __restrict__ kept, const unsigned long long* __restrict__ sorted, long long n,
              long long m, unsigned long long* __restrict__ r2) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const unsigned long long key = kept[e];
    unsigned long long r = 0ull;
    if (key != NA_KEY) {
      long long lo = 0, hi = m;           // the first position whose key is not below `key`
      while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
      }
      // the first position whose key is above `key`: sorted[lo] is the key itself and a run of equal keys is short next
      // to the plane, so the bracket is found by doubling steps from lo (the same cache line for a run of one) before it
      // is halved
      long long a = lo + 1, b = m, step = 1;
      while (a + step <= m && sorted[a + step - 1] <= key) { a += step; step <<= 1; }
      if (a + step - 1 < b) b = a + step - 1;
      while (a < b) {
        const long long mid = a + ((b - a) >> 1);
        if (sorted[mid] <= key) a = mid + 1; else b = mid;
      }
      r = (unsigned long long)(2 * m - lo - a + 1);
    }
    r2[e] = r;
  }
}

// ---- the observed labelling per class -------------------------------------------------------------------------------

// One workgroup per row i (grid-stride): the values (i, j), j > i, with cls[j] == cls[i] add their r2 to class_w2 and
// count into class_nw of that class.  The class is the row's, so a row costs one pair of atomics.
__global__ void __launch_bounds__(CT)
k_anosim_classes(const unsigned long long* __restrict__ r2, const int32_t* __restrict__ cls, int S,
                 unsigned long long* __restrict__ class_w2, unsigned long long* __restrict__ class_nw) {
  __shared__ unsigned long long sh[4];
  const int tid = (int)threadIdx.x;
  for (int i = (int)blockIdx.x; i < S - 1; i += (int)gridDim.x) {
    const int c = cls[i];
    const long long row = (long long)i * (2ll * S - i - 1) / 2 - i - 1;   // + j: the pair (i, j)
    unsigned long long w = 0ull, k = 0ull;
    for (int j = i + 1 + tid; j < S; j += CT) {
      const unsigned long long r = r2[row + j];
      if (cls[j] == c && r != 0ull) { w += r; ++k; }
    }
    w = block_reduce(w, sh, Add());
    k = block_reduce(k, sh, Add());
    if (tid == 0 && k) {
      atomicAdd(&class_w2[c], w);
      atomicAdd(&class_nw[c], k);
    }
  }
}

// ---- the permutation kernel ----------------------------------------------------------------------------------------

// labT [groups][S][ANO_PB] halfwords: the labels of ANO_PB labellings side by side per sample, so that the ANO_PB
// labels of a row are 32 consecutive bytes at an address the whole workgroup shares -- scalar loads -- and the
// ANO_PB labels of a thread's column two 16-byte loads into registers that stay for the whole run of rows.
//
// A workgroup (blockIdx.x: group of labellings, .y: column strip, .z: run of rows) owns the columns [j0, j0 + T) of
// the triangle, the rows [i0, i0 + RR) and ANO_PB labellings.  It takes its strip 256 columns at a time: thread t
// holds column j = c0 + t with that column's labels in registers, and walks the rows i < j of its run; the 256
// threads read r2[row_offset(S, i) + j - i - 1] of consecutive j: one coalesced read per row.  Per labelling a thread
// keeps a 64-bit sum of r2 and, with NW, a 32-bit count; `match ? r2 : 0` is a compare and two selects.  Threads with
// j <= i (the rows that cross the diagonal) or j past the strip read nothing and add 0; an NA pair has r2 = 0 and adds
// 0.  NW = false (no NA pair in the plane): nW is a function of the class sizes, the host's.  At the end: a workgroup
// reduction and one 64-bit atomicAdd per labelling into w2 / nw [groups][ANO_PB] (the caller zeroes them).  The group
// is the grid's fastest dimension: the workgroups that read the same tile of r2 run side by side and share it in L2.
template <bool NW>
__global__ void __launch_bounds__(256)
k_anosim_perm(const unsigned long long* __restrict__ r2, const uint16_t* __restrict__ labT, int S, int T, int RR,
              unsigned long long* __restrict__ w2, unsigned long long* __restrict__ nw) {
  __shared__ unsigned long long s_w[4][ANO_PB];
  __shared__ unsigned int s_n[4][ANO_PB];
  const int tid = (int)threadIdx.x;
  const int j0 = (int)blockIdx.y * T;
  const int jend = j0 + T < S ? j0 + T : S;
  const int i0 = (int)blockIdx.z * RR;
  const int i1 = i0 + RR < jend - 1 ? i0 + RR : jend - 1;   // rows i <= jend - 2 have a column of the strip
  if (i0 >= i1) return;                                      // (the same for every thread of the workgroup)
  const uint16_t* __restrict__ lab = labT + (size_t)blockIdx.x * (size_t)S * ANO_PB;
  unsigned long long acc[ANO_PB];
  unsigned int cnt[ANO_PB];
#pragma unroll
  for (int p = 0; p < ANO_PB; ++p) { acc[p] = 0ull; cnt[p] = 0u; }
  for (int c0 = j0; c0 < jend; c0 += 256) {
    const int j = c0 + tid;
    const bool col = j < jend;
    if (c0 + 255 <= i0) continue;   // every column of the chunk lies at or below the run's first row
    uint32_t cl[ANO_PB];
    {
      const uint4* q = reinterpret_cast<const uint4*>(lab + (size_t)(col ? j : 0) * ANO_PB);
#pragma unroll
      for (int v = 0; v < ANO_PB / 8; ++v) {
        const uint4 u = q[v];
        cl[8 * v + 0] = u.x & 0xFFFFu; cl[8 * v + 1] = u.x >> 16;
        cl[8 * v + 2] = u.y & 0xFFFFu; cl[8 * v + 3] = u.y >> 16;
        cl[8 * v + 4] = u.z & 0xFFFFu; cl[8 * v + 5] = u.z >> 16;
        cl[8 * v + 6] = u.w & 0xFFFFu; cl[8 * v + 7] = u.w >> 16;
      }
    }
    const int cend = c0 + 256 < jend ? c0 + 256 : jend;
    const int iend = i1 < cend - 1 ? i1 : cend - 1;          // rows below the chunk's last column
    long long at = (long long)i0 * (2ll * S - i0 - 1) / 2 - i0 - 1 + j;   // the pair (i, j) of row i = i0
    unsigned long long ahead = (col && j > i0 && i0 < iend) ? r2[at] : 0ull;   // a row's rank is read one row ahead
    for (int i = i0; i < iend; ++i) {
      const uint4* q = reinterpret_cast<const uint4*>(lab + (size_t)i * ANO_PB);   // (uniform: scalar loads)
      const unsigned long long r = ahead;
      at += S - i - 2;                                                             // the pair (i + 1, j)
      ahead = (col && j > i + 1 && i + 1 < iend) ? r2[at] : 0ull;
#pragma unroll
      for (int v = 0; v < ANO_PB / 8; ++v) {
        const uint4 u = q[v];
        const uint32_t rl[8] = {u.x & 0xFFFFu, u.x >> 16, u.y & 0xFFFFu, u.y >> 16,
                                u.z & 0xFFFFu, u.z >> 16, u.w & 0xFFFFu, u.w >> 16};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const bool match = cl[8 * v + k] == rl[k];
          acc[8 * v + k] += match ? r : 0ull;
          if (NW) cnt[8 * v + k] += (match && r != 0ull) ? 1u : 0u;
        }
      }
    }
  }
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int p = 0; p < ANO_PB; ++p) {
    unsigned long long a = acc[p];
    unsigned int c = cnt[p];
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      if (NW) c += __shfl_xor(c, o, 64);
    }
    if (lane == 0) { s_w[w][p] = a; s_n[w][p] = c; }
  }
  __syncthreads();
  if (tid < ANO_PB) {
    const unsigned long long a = s_w[0][tid] + s_w[1][tid] + s_w[2][tid] + s_w[3][tid];
    const size_t slot = (size_t)blockIdx.x * ANO_PB + (size_t)tid;
    if (a) atomicAdd(&w2[slot], a);
    if (NW) {
      const unsigned long long c = (unsigned long long)s_n[0][tid] + s_n[1][tid] + s_n[2][tid] + s_n[3][tid];
      if (c) atomicAdd(&nw[slot], c);
    }
  }
}

}  // namespace

hipError_t launch_anosim_count(const unsigned long long* kept, long long n, unsigned long long* total,
                               unsigned long long* dhist, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  (void)hipGetLastError();
  const long long want = (n + 255) / 256;
  hipLaunchKernelGGL(k_anosim_count, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, s, kept, n, total, dhist);
  return hipGetLastError();
}

hipError_t launch_anosim_rank(const unsigned long long* kept, const unsigned long long* sorted, long long n, long long m,
                              unsigned long long* r2, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (m < 0 || m > n || r2 == sorted) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const long long want = (n + 255) / 256;
  hipLaunchKernelGGL(k_anosim_rank, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, s, kept, sorted, n, m, r2);
  return hipGetLastError();
}

hipError_t launch_anosim_classes(const unsigned long long* r2, const int32_t* cls, int S, unsigned long long* class_w2,
                                 unsigned long long* class_nw, hipStream_t s) {
  if (S < 2) return hipSuccess;
  if (S > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_anosim_classes, dim3((unsigned)(S - 1 < 4096 ? S - 1 : 4096)), dim3(CT), 0, s, r2, cls, S, class_w2,
                     class_nw);
  return hipGetLastError();
}

hipError_t launch_anosim_perm(const unsigned long long* r2, const uint16_t* labT, int S, int n_groups, int strip,
                              int count_nw, unsigned long long* w2, unsigned long long* nw, hipStream_t s) {
  if (S < 2 || n_groups <= 0) return hipSuccess;
  if (S > 65535 || strip < ANO_STRIP_MIN || strip > ANO_STRIP_MAX) return hipErrorInvalidValue;
  const int n_strips = (S + strip - 1) / strip;
  const int n_runs = (S - 1 + ANO_ROW_RUN - 1) / ANO_ROW_RUN;
  if (n_strips > 65535 || n_runs > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const dim3 grid((unsigned)n_groups, (unsigned)n_strips, (unsigned)n_runs);
  if (count_nw)
    hipLaunchKernelGGL(k_anosim_perm<true>, grid, dim3(256), 0, s, r2, labT, S, strip, ANO_ROW_RUN, w2, nw);
  else
    hipLaunchKernelGGL(k_anosim_perm<false>, grid, dim3(256), 0, s, r2, labT, S, strip, ANO_ROW_RUN, w2, nw);
  return hipGetLastError();
}

}  // namespace icikt
