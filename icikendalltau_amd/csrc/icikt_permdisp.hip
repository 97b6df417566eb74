// icikt_permdisp.hip -- PERMDISP (Anderson 2006; vegan::betadisper + permutest) of the samples' classes under the
// dissimilarity 1 - raw: every sample's sum of squared dissimilarities to every class, on the device
// (icikt_permdisp_f64, host side: icikt_capi_permdisp.cpp).
//
// The rule.  A pair i < j is a VALUE iff its raw is not NA (reason code 0: k_median_keep's rule).  A value's squared
// dissimilarity is the integer q = fixed::quantise_key(key) of its kept key (icikt_fixed.h: PERMANOVA's q, in 0 ..
// 2^52); a pair that is no value adds 0.  T[i][c] is the sum of q_ij over the samples j != i of class c, for every
// sample i and every class c in 0 .. n_class - 1; an empty class has 0.  Q is the sum of q over all pairs and n_na the
// pairs that are no value: bit for bit k_pmv_quant's on the same plane.  Everything behind the quantisation is an
// integer sum, so the result is a pure function of the input, whatever the block cut, the bin path or the order in
// which the atomics land.  What follows from the table -- A_c = 1/2 sum_{i in c} T[i][c], X[i][c] = n_c T[i][c] - A_c,
// the distance sqrt(|X|) / (n_c 2^25) of sample i to the centroid of class c, the ANOVA F of the own-class distances
// and its permutation test -- is the front end's, in integers and fractions.
//
// The pair engine runs the combn triangle in blocks of whole rows; after each block k_median_keep (icikt_medians.hip)
// writes the block's keys into the kept plane.  After the last block ONE kernel sweeps the plane:
//   k_disp_table   one workgroup per sample s, k_mst_best's addressing: the partners t > s are row s of the triangle,
//                  contiguous in t; the partners t < s are column s, one key per row t, strided.  Each partner's q goes,
//                  as its two limbs, into the bins of the partner's class.  There is no second plane: q is two double
//                  operations and a conversion per key, made on the fly (8 bytes per pair where PERMANOVA has 16).
// The bins of a sample are 2 n_class words.  LDS: up to PMV_LDS_CLASSES classes they are kept in LDS (16 bytes a class,
// 32 KB), zeroed, added to with LDS atomics and stored once to t_lo / t_hi [s][.]; above that they are global atomics
// on the sample's own row of the table, which the host has zeroed -- no other workgroup touches that row.  In the row
// role only (t > s, every pair once) the workgroup also counts the NA_KEY pairs and sums the limbs of q: one atomic
// each per workgroup on totals[PMV_T_NA / _LO / _HI].  No kernel waits on another workgroup.
//
// ONE CLASS IN A WAVE.  With few classes 64 lanes queue on two LDS words, and LDS atomics on one address serialise.
// When a ballot shows that every partner of the wave's 64 has the same class -- a class-sorted cohort almost always --
// the wave adds its limbs up with shuffles and one lane issues the two atomics.  The sums are of integers: which path a
// wave takes cannot change a bit.  (Measured at S = 4 096: 0.147 ms class-sorted against 0.151 ms interleaved, and
// 0.154 ms with 2 048 classes; the column role's strided reads, a 128-byte line per key, are what the time is.  DESIGN.md
// section 26 has the figures.)
//
// THE ACCUMULATORS (q <= 2^52, S <= 65 535, P = S (S - 1) / 2 < 2^31)
//   a cell of the bins / of t_lo, t_hi   at most S - 1 values of lo < 2^32 and hi <= 2^20: below 2^48 and 2^36.
//                                        T = hi 2^32 + lo < 2^68
//   a wave's sum (one class in a wave)   64 such limbs: below 2^38 and 2^26
//   a thread's row-role totals           at most ceil(S / 256) = 256 values: below 2^40 and 2^28; the workgroup's below
//                                        2^48 and 2^36; totals[] over the P pairs of the grid below 2^63 and 2^51
//                                        (k_pmv_quant's bound)
// Every sum is of non-negative integers and never wraps, so the order of the atomic additions does not show.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_fixed.h"

namespace icikt {

namespace {

using namespace colsort;

// first pair of row i of combn(S, 2) (cut_rows' formula, icikt_blocks.h)
__device__ __forceinline__ long long disp_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One workgroup per sample s = blockIdx.x.  cls [S] in 0 .. n_class - 1 (the host has checked every label).
// LDS: t_lo / t_hi [s][0 .. n_class) are stored, every cell; otherwise they are added to (the caller zeroes them).
// totals: PMV_TOTALS words, added to (the caller zeroes them).
template <bool LDS>
__global__ void __launch_bounds__(CT)
k_disp_table(const unsigned long long* __restrict__ kept, const int32_t* __restrict__ cls, int S, int n_class,
             unsigned long long* __restrict__ t_lo, unsigned long long* __restrict__ t_hi,
             unsigned long long* __restrict__ totals) {
  extern __shared__ unsigned long long s_bins[];   // LDS: [2][n_class]
  __shared__ unsigned long long sh[4];
  __shared__ unsigned int s_na;
  const int tid = (int)threadIdx.x;
  const int s = (int)blockIdx.x;
  if (s >= S) return;                                  // (the same for every thread of the workgroup)
  unsigned long long* lo = LDS ? s_bins : t_lo + (size_t)s * (size_t)n_class;
  unsigned long long* hi = LDS ? s_bins + n_class : t_hi + (size_t)s * (size_t)n_class;
  if (tid == 0) s_na = 0u;
  if (LDS)
    for (int c = tid; c < 2 * n_class; c += CT) s_bins[c] = 0ull;
  __syncthreads();
  const long long row_s = disp_rowoff(S, s) - s - 1;   // + t: the pair (s, t), t > s
  unsigned int na = 0u;
  unsigned long long tot_lo = 0ull, tot_hi = 0ull;
  for (int base = 0; base < S; base += CT) {           // (every thread runs every round: the ballots and shuffles below)
    const int t = base + tid;
    const bool in = t < S && t != s;
    unsigned long long key = 0ull;
    int c = 0;
    if (in) {
      key = t > s ? kept[row_s + t] : kept[disp_rowoff(S, t) + (s - t - 1)];
      c = (int)cls[t];
    }
    const bool row = in && t > s;
    na += (unsigned int)__popcll(__ballot(row && key == NA_KEY));
    const unsigned long long v = in ? fixed::quantise_key(key) : 0ull;
    const unsigned long long vl = fixed::limb_lo(v), vh = fixed::limb_hi(v);
    if (row) { tot_lo += vl; tot_hi += vh; }
    const unsigned long long active = __ballot(in);
    if (active == 0ull) continue;                      // (the same for every lane of the wave)
    const int first = __ffsll((long long)active) - 1;
    const int c0 = __shfl(c, first, 64);
    if (__ballot(in && c != c0) == 0ull) {             // one class in the wave: one lane adds the wave's sums
      const unsigned long long wl = wave_sum(vl), wh = wave_sum(vh);
      if ((tid & 63) == first) {
        if (wl) atomicAdd(&lo[c0], wl);
        if (wh) atomicAdd(&hi[c0], wh);
      }
    } else if (in) {
      if (vl) atomicAdd(&lo[c], vl);
      if (vh) atomicAdd(&hi[c], vh);
    }
  }
  if ((tid & 63) == 0) atomicAdd(&s_na, na);           // the ballots gave every lane the wave's count
  tot_lo = block_reduce(tot_lo, sh, Add());
  tot_hi = block_reduce(tot_hi, sh, Add());            // (its barriers order s_na and the bins as well)
  if (tid == 0) {
    if (s_na) atomicAdd(&totals[PMV_T_NA], (unsigned long long)s_na);
    if (tot_lo) atomicAdd(&totals[PMV_T_LO], tot_lo);
    if (tot_hi) atomicAdd(&totals[PMV_T_HI], tot_hi);
  }
  if (LDS) {
    for (int c = tid; c < n_class; c += CT) {
      t_lo[(size_t)s * (size_t)n_class + c] = s_bins[c];
      t_hi[(size_t)s * (size_t)n_class + c] = s_bins[n_class + c];
    }
  }
}

}  // namespace

hipError_t launch_disp_table(const unsigned long long* kept, const int32_t* cls, int S, int n_class,
                             unsigned long long* t_lo, unsigned long long* t_hi, unsigned long long* totals,
                             hipStream_t s) {
  if (S <= 0) return hipSuccess;
  if (S > 65535 || n_class < 1 || n_class > 65535 || (long long)S * n_class > DISP_MAX_CELLS) return hipErrorInvalidValue;
  (void)hipGetLastError();
  if (n_class <= PMV_LDS_CLASSES) {
    hipLaunchKernelGGL(k_disp_table<true>, dim3((unsigned)S), dim3(CT), 2 * (size_t)n_class * sizeof(unsigned long long), s,
                       kept, cls, S, n_class, t_lo, t_hi, totals);
  } else {
    const size_t bytes = (size_t)S * (size_t)n_class * sizeof(unsigned long long);
    hipError_t e = hipMemsetAsync(t_lo, 0, bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(t_hi, 0, bytes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_disp_table<false>, dim3((unsigned)S), dim3(CT), 0, s, kept, cls, S, n_class, t_lo, t_hi, totals);
  }
  return hipGetLastError();
}

}  // namespace icikt
