// icikt_permanova.hip -- PERMANOVA (Anderson 2001; vegan::adonis2) of the samples' classes under the dissimilarity
// 1 - raw: the sums of squared dissimilarities per class and labelling, on the device (icikt_permanova_f64, host side:
// icikt_capi_permanova.cpp).
//
// The rule.  A pair i < j is a VALUE iff its raw is not NA (reason code 0: k_median_keep's rule).  A value's squared
// dissimilarity is summed as the integer q = fixed::quantise(raw) = llrint(ldexp((1 - raw)^2, 50)) of icikt_fixed.h, in
// 0 .. 2^52; a pair that is no value has q = 0.  Q is the sum of q over all pairs; for a labelling L (a class index per
// sample) and a class c, A_c(L) is the sum of q over the pairs whose two samples both have class c.  Everything behind
// the quantisation is an integer sum: the result is a pure function of the input and the labellings, whatever the
// block cut, the strip, the batch, the grid or the order in which the atomics land.  The statistic (the 1 / n_c
// weights, F, R2 and the comparison of labellings) is the front end's, in fractions.
//
// The pair engine runs the combn triangle in blocks of whole rows; after each block k_median_keep (icikt_medians.hip)
// writes the block's keys into the kept plane.  After the last block
//   k_pmv_quant    one pass over the plane: q per pair, the NA pairs' count and Q;
//   k_pmv_perm     the hot path: per column j and labelling, the sum of q over the rows i < j of j's class -- ANO_PB
//                  labellings at a time, k_anosim_perm's geometry;
//   k_pmv_classes  per labelling, the columns' sums into the bins of the columns' classes.
// No kernel waits on another workgroup.
//
// THE ACCUMULATORS (q <= 2^52, S <= 65 535, P = S (S - 1) / 2 < 2^31)
//   a thread of k_pmv_quant     the two limbs of its q apart: lo < 2^32 and hi <= 2^20 per value, at most P values in the
//                               whole grid: below 2^63 and 2^51, and so are the workgroup's sums and the totals
//   acc[p] of k_pmv_perm        one 256-column chunk of one run: at most PMV_ROW_RUN = 1 024 values: below 2^62
//   colsum_lo / colsum_hi       the limbs (low 32 bits, the rest: below 2^30) of those sums over the at most
//                               ceil(S / 1 024) = 64 runs of a column: below 2^38 and 2^36
//   bins_lo / bins_hi           the columns' limb sums over at most S columns: below 2^54 and 2^52.  A = hi 2^32 + lo.
// Every sum is of non-negative integers and never wraps, so the order of the atomic additions does not show.
//
// THE RUN OF ROWS.  k_anosim_perm's run is 256 rows; with that run k_pmv_perm took 3.09 ms where k_anosim_perm takes
// 1.21 ms (S = 4 096, 999 permutations, a kernel trace), and the difference was the column-sum atomics: their number
// is columns x runs x labellings x 2.  Runs of 512 rows gave 1.68 ms and runs of 1 024 rows 1.31 ms for both labelling
// kernels, with identical sums; 1 024 it is (DESIGN.md section 25 has the figures).  A call of one group of labellings
// has a quarter of the workgroups for it and takes 0.35 ms longer behind a 30 ms pair kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_fixed.h"

// rows of a workgroup's run in k_pmv_perm (a development build may set another: at most 4 095, so that acc stays below 2^64)
#ifndef ICIKT_PMV_ROW_RUN
#define ICIKT_PMV_ROW_RUN 1024
#endif

namespace icikt {

namespace {

using namespace colsort;

constexpr int PMV_ROW_RUN = ICIKT_PMV_ROW_RUN;
static_assert(PMV_ROW_RUN >= 1 && PMV_ROW_RUN <= 4095, "acc[p] of k_pmv_perm: a run's values of at most 2^52 in 64 bits");

// ---- quant: q of every pair, the NA pairs and Q -------------------------------------------------------------------

// totals[PMV_T_NA] += the NA_KEY pairs, totals[PMV_T_LO] / [PMV_T_HI] += the limbs of every q (the caller zeroes them)
__global__ void __launch_bounds__(CT)
k_pmv_quant(const unsigned long long* __restrict__ kept, long long n, unsigned long long* __restrict__ q,
            unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long sh[4];
  __shared__ unsigned int s_na;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_na = 0u;
  __syncthreads();
  unsigned int na = 0u;
  unsigned long long lo = 0ull, hi = 0ull;
  for (long long base = (long long)blockIdx.x * CT; base < n; base += (long long)gridDim.x * CT) {
    const long long e = base + tid;
    const bool in = e < n;
    const unsigned long long key = in ? kept[e] : 0ull;
    na += (unsigned int)__popcll(__ballot(in && key == NA_KEY));
    if (in) {
      const unsigned long long v = fixed::quantise_key(key);
      q[e] = v;
      lo += fixed::limb_lo(v);
      hi += fixed::limb_hi(v);
    }
  }
  if ((tid & 63) == 0) atomicAdd(&s_na, na);   // the ballots gave every lane the wave's count
  lo = block_reduce(lo, sh, Add());
  hi = block_reduce(hi, sh, Add());            // (its barriers order s_na as well)
  if (tid == 0) {
    if (s_na) atomicAdd(&totals[PMV_T_NA], (unsigned long long)s_na);
    if (lo) atomicAdd(&totals[PMV_T_LO], lo);
    if (hi) atomicAdd(&totals[PMV_T_HI], hi);
  }
}

// ---- the permutation kernel ----------------------------------------------------------------------------------------

// labT [groups][S][ANO_PB] halfwords, the grid (group of labellings, column strip, run of rows), the 256-column chunks,
// the labels of a thread's column in registers, the row's labels by scalar loads and q read coalesced one row ahead:
// all k_anosim_perm's (icikt_anosim.hip says why).  What differs is where a thread's sums go.  Under labelling p the
// sum of thread t belongs to the class of ITS column, so the workgroup has no common sum to reduce to; binning by class
// here would queue 256 threads x ANO_PB labellings on as few addresses as there are classes.  Instead, at the end of a
// chunk, every thread adds the two limbs of acc[p] to colsum_lo / colsum_hi [group][S][ANO_PB] at its own column: one
// address per thread and labelling, consecutive threads 128 bytes apart, contended only by the workgroups of the other
// row runs of the same column (at most ceil(S / PMV_ROW_RUN)).  acc is cleared per chunk, for the next chunk is another column.
__global__ void __launch_bounds__(256)
k_pmv_perm(const unsigned long long* __restrict__ q, const uint16_t* __restrict__ labT, int S, int T, int RR,
           unsigned long long* __restrict__ colsum_lo, unsigned long long* __restrict__ colsum_hi) {
  const int tid = (int)threadIdx.x;
  const int j0 = (int)blockIdx.y * T;
  const int jend = j0 + T < S ? j0 + T : S;
  const int i0 = (int)blockIdx.z * RR;
  const int i1 = i0 + RR < jend - 1 ? i0 + RR : jend - 1;   // rows i <= jend - 2 have a column of the strip
  if (i0 >= i1) return;                                      // (the same for every thread of the workgroup)
  const uint16_t* __restrict__ lab = labT + (size_t)blockIdx.x * (size_t)S * ANO_PB;
  for (int c0 = j0; c0 < jend; c0 += 256) {
    const int j = c0 + tid;
    const bool col = j < jend;
    if (c0 + 255 <= i0) continue;   // every column of the chunk lies at or below the run's first row
    unsigned long long acc[ANO_PB];
#pragma unroll
    for (int p = 0; p < ANO_PB; ++p) acc[p] = 0ull;
    uint32_t cl[ANO_PB];
    {
      const uint4* w = reinterpret_cast<const uint4*>(lab + (size_t)(col ? j : 0) * ANO_PB);
#pragma unroll
      for (int v = 0; v < ANO_PB / 8; ++v) {
        const uint4 u = w[v];
        cl[8 * v + 0] = u.x & 0xFFFFu; cl[8 * v + 1] = u.x >> 16;
        cl[8 * v + 2] = u.y & 0xFFFFu; cl[8 * v + 3] = u.y >> 16;
        cl[8 * v + 4] = u.z & 0xFFFFu; cl[8 * v + 5] = u.z >> 16;
        cl[8 * v + 6] = u.w & 0xFFFFu; cl[8 * v + 7] = u.w >> 16;
      }
    }
    const int cend = c0 + 256 < jend ? c0 + 256 : jend;
    const int iend = i1 < cend - 1 ? i1 : cend - 1;          // rows below the chunk's last column
    long long at = (long long)i0 * (2ll * S - i0 - 1) / 2 - i0 - 1 + j;   // the pair (i, j) of row i = i0
    unsigned long long ahead = (col && j > i0 && i0 < iend) ? q[at] : 0ull;   // a row's q is read one row ahead
    for (int i = i0; i < iend; ++i) {
      const uint4* w = reinterpret_cast<const uint4*>(lab + (size_t)i * ANO_PB);   // (uniform: scalar loads)
      const unsigned long long r = ahead;
      at += S - i - 2;                                                             // the pair (i + 1, j)
      ahead = (col && j > i + 1 && i + 1 < iend) ? q[at] : 0ull;
#pragma unroll
      for (int v = 0; v < ANO_PB / 8; ++v) {
        const uint4 u = w[v];
        const uint32_t rl[8] = {u.x & 0xFFFFu, u.x >> 16, u.y & 0xFFFFu, u.y >> 16,
                                u.z & 0xFFFFu, u.z >> 16, u.w & 0xFFFFu, u.w >> 16};
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[8 * v + k] += (cl[8 * v + k] == rl[k]) ? r : 0ull;
      }
    }
    if (col) {   // (j < jend <= S: inside the group's S x ANO_PB slots)
      const size_t slot = ((size_t)blockIdx.x * (size_t)S + (size_t)j) * ANO_PB;
#pragma unroll
      for (int p = 0; p < ANO_PB; ++p) {
        const unsigned long long a = acc[p];
        if (a) {
          atomicAdd(&colsum_lo[slot + p], fixed::limb_lo(a));
          atomicAdd(&colsum_hi[slot + p], fixed::limb_hi(a));
        }
      }
    }
  }
}

// ---- the columns' sums into the bins of their classes ----------------------------------------------------------------

// One workgroup per labelling l = blockIdx.x (group l / ANO_PB, slot l % ANO_PB): bins[l][c] += colsum[j] over the
// columns j whose label under l is c.  S additions per labelling where the hot kernel has S^2 / 2, so that few classes
// -- many columns per address -- cost little next to it.  LDS: the bins of a labelling are kept in LDS (n_class <=
// PMV_LDS_CLASSES: 16 bytes each, 32 KB), added to with LDS atomics and stored once; otherwise they are added to in
// global memory, where the many classes keep the columns per address few.  Labels are below n_class: the host has
// checked every one before its batch is uploaded, and the unused slots of a last group are labelling 0s.
template <bool LDS>
__global__ void __launch_bounds__(256)
k_pmv_classes(const uint16_t* __restrict__ labT, const unsigned long long* __restrict__ colsum_lo,
              const unsigned long long* __restrict__ colsum_hi, int S, int n_class,
              unsigned long long* __restrict__ bins_lo, unsigned long long* __restrict__ bins_hi) {
  extern __shared__ unsigned long long s_bins[];   // LDS: [2][n_class]
  const int tid = (int)threadIdx.x;
  const size_t l = blockIdx.x;
  const size_t from = (l / ANO_PB) * (size_t)S * ANO_PB + (l % ANO_PB);
  unsigned long long* lo = LDS ? s_bins : bins_lo + l * (size_t)n_class;
  unsigned long long* hi = LDS ? s_bins + n_class : bins_hi + l * (size_t)n_class;
  if (LDS) {
    for (int c = tid; c < 2 * n_class; c += 256) s_bins[c] = 0ull;
    __syncthreads();
  }
  for (int j = tid; j < S; j += 256) {
    const size_t at = from + (size_t)j * ANO_PB;
    const unsigned long long a = colsum_lo[at], b = colsum_hi[at];
    if (a | b) {
      const int c = (int)labT[at];
      atomicAdd(&lo[c], a);
      atomicAdd(&hi[c], b);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int c = tid; c < n_class; c += 256) {
      bins_lo[l * (size_t)n_class + c] = s_bins[c];
      bins_hi[l * (size_t)n_class + c] = s_bins[n_class + c];
    }
  }
}

}  // namespace

hipError_t launch_pmv_quant(const unsigned long long* kept, long long n, unsigned long long* q,
                            unsigned long long* totals, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (q == kept) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const long long want = (n + CT - 1) / CT;
  hipLaunchKernelGGL(k_pmv_quant, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(CT), 0, s, kept, n, q, totals);
  return hipGetLastError();
}

hipError_t launch_pmv_perm(const unsigned long long* q, const uint16_t* labT, int S, int n_groups, int strip,
                           unsigned long long* colsum_lo, unsigned long long* colsum_hi, hipStream_t s) {
  if (S < 2 || n_groups <= 0) return hipSuccess;
  if (S > 65535 || strip < ANO_STRIP_MIN || strip > ANO_STRIP_MAX) return hipErrorInvalidValue;
  const int n_strips = (S + strip - 1) / strip;
  const int n_runs = (S - 1 + PMV_ROW_RUN - 1) / PMV_ROW_RUN;
  if (n_strips > 65535 || n_runs > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const dim3 grid((unsigned)n_groups, (unsigned)n_strips, (unsigned)n_runs);
  hipLaunchKernelGGL(k_pmv_perm, grid, dim3(256), 0, s, q, labT, S, strip, PMV_ROW_RUN, colsum_lo, colsum_hi);
  return hipGetLastError();
}

hipError_t launch_pmv_classes(const uint16_t* labT, const unsigned long long* colsum_lo,
                              const unsigned long long* colsum_hi, int S, int n_class, long long n_lab,
                              unsigned long long* bins_lo, unsigned long long* bins_hi, hipStream_t s) {
  if (S < 1 || n_lab <= 0) return hipSuccess;
  if (S > 65535 || n_class < 1 || n_class > 65535 || n_lab > ANO_PERMS_MAX) return hipErrorInvalidValue;
  (void)hipGetLastError();
  if (n_class <= PMV_LDS_CLASSES)
    hipLaunchKernelGGL(k_pmv_classes<true>, dim3((unsigned)n_lab), dim3(256),
                       2 * (size_t)n_class * sizeof(unsigned long long), s, labT, colsum_lo, colsum_hi, S, n_class, bins_lo,
                       bins_hi);
  else
    hipLaunchKernelGGL(k_pmv_classes<false>, dim3((unsigned)n_lab), dim3(256), 0, s, labT, colsum_lo, colsum_hi, S,
                       n_class, bins_lo, bins_hi);
  return hipGetLastError();
}

}  // namespace icikt
