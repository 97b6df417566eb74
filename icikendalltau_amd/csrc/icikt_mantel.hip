// icikt_mantel.hip -- the Mantel test (Mantel 1967; vegan::mantel, skbio.stats.distance.mantel) of the dissimilarity
// 1 - raw against ANOTHER matrix of the same samples, with its permutation test, on the device (icikt_mantel_f64, host
// side: icikt_capi_mantel.cpp).
//
// The rule.  S samples, P = S (S - 1) / 2 pairs i < j in combn order.  x comes from the data matrix, y from `other`, one
// finite double per pair.  Both become unsigned integers below 2^32:
//   method spearman   the doubled average rank among the P values, ascending in value.  For x the order is ascending
//                     1 - raw: k_anosim_rank's r2 with M = P (-0 equals +0).  For y it is lo + hi + 1, lo the values
//                     below and hi the values at or below: k_anosim_rank over the keys of -y gives exactly that
//                     (2 P - #above - #at-or-above + 1 = #at-or-below + #below + 1).  2 P < 2^32 for S <= 65 535
//   method pearson    xv = llrint(ldexp(1.0 - raw, 30)) and yv = llrint(ldexp(y - lo, 31 - e)), both in 0 .. 2^31
//                     (icikt_mantel.h states the rule and holds the code)
// For a permutation pi of the samples T(pi) = sum over i < j of xv_ij yv_{pi(i) pi(j)}; the observed T is T of the
// identity, labelling 0 of the same kernel.  A product is below 2^64: its low 32 bits and the rest are summed apart
// (two limbs, T = hi 2^32 + lo).  The moments sum v, sum v^2 of either vector are limbs too.  A pair whose raw is NA
// leaves nothing to sum: the host launches no labelling then.  Everything here is an integer sum: the result is a pure
// function of the input, `other` and the permutations, whatever the block cut, the sort's tile, the strip, the batch or
// the grid.  A 0/1 design matrix gives many exactly equal T; that case is why the sums are integers.
//
//   k_mantel_ykeys     `other` (P doubles in the kept plane) into the sortable keys of -y, in place (spearman);
//   k_mantel_yquant    `other` into yv (pearson);
//   k_mantel_expand    a plane of y values into the symmetric S x S table of 32-bit words, zero diagonal;
//   k_mantel_xquant    the kept keys into xv, and the NA pairs' count (pearson);
//   k_mantel_moments   sum v and sum v^2 of a plane, as limbs;
//   k_mantel_perm      the hot path: T of ANO_PB permutations at a time, see below.
// No kernel waits on another workgroup.
//
// THE ACCUMULATORS (v < 2^32, S <= 65 535, P < 2^31)
//   k_mantel_moments           v and v^2 split into limbs below 2^32, at most P of them in the whole grid: every sum is
//                              below 2^63
//   acc_lo / acc_hi of k_mantel_perm   a thread adds one limb below 2^32 per row and chunk: at most MANTEL_ROW_RUN rows
//                              x ANO_STRIP_MAX / 256 = 16 chunks: below 2^46; the workgroup's sum below 2^54
//   t_lo / t_hi                the limbs of at most P products: below 2^63.  T = hi 2^32 + lo < 2^95.
// Every sum is of non-negative integers and never wraps, so the order of the atomic additions does not show.
//
// THE GATHER.  The table is 4 S^2 bytes: 64 MB at S = 4 096 (it stays in the 256 MB last-level cache; the 16 rows a
// workgroup reads at a time, 256 KB, in the XCD's 4 MB L2) and 4 GB at S = 32 768 (HBM; a row is 128 KB).  Every index
// the gather follows was range-checked on the host before its upload and is compared with S again here: one that is
// not below S reads row or column 0, never past the table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_mantel.h"

namespace icikt {

namespace {

using namespace colsort;

// ---- y: keys, fixed-point values, the table --------------------------------------------------------------------------

// plane[e] holds a finite double y: it becomes cor_key(-y), so that an ascending sort is descending in y
__global__ void __launch_bounds__(CT)
k_mantel_ykeys(unsigned long long* __restrict__ plane, long long n) {
  for (long long e = (long long)blockIdx.x * CT + threadIdx.x; e < n; e += (long long)gridDim.x * CT)
    plane[e] = cor_key(-__longlong_as_double((long long)plane[e]));
}

__global__ void __launch_bounds__(CT)
k_mantel_yquant(const unsigned long long* __restrict__ y, long long n, double lo, int ex,
                unsigned long long* __restrict__ yv) {
  for (long long e = (long long)blockIdx.x * CT + threadIdx.x; e < n; e += (long long)gridDim.x * CT)
    yv[e] = mantel::quantise_y(__longlong_as_double((long long)y[e]), lo, ex);
}

// One workgroup per row i (grid-stride over 0 .. S - 1): tab[i][j] = tab[j][i] = the low word of plane[(i, j)], j > i,
// and tab[i][i] = 0.  The row is read and written coalesced, its mirror image strided: once per call.
__global__ void __launch_bounds__(CT)
k_mantel_expand(const unsigned long long* __restrict__ plane, int S, uint32_t* __restrict__ tab) {
  const int tid = (int)threadIdx.x;
  for (int i = (int)blockIdx.x; i < S; i += (int)gridDim.x) {
    const long long row = (long long)i * (2ll * S - i - 1) / 2 - i - 1;   // + j: the pair (i, j)
    if (tid == 0) tab[(size_t)i * (size_t)S + (size_t)i] = 0u;
    for (int j = i + 1 + tid; j < S; j += CT) {
      const uint32_t v = (uint32_t)plane[row + j];
      tab[(size_t)i * (size_t)S + (size_t)j] = v;
      tab[(size_t)j * (size_t)S + (size_t)i] = v;
    }
  }
}

// ---- x: fixed-point values and the NA pairs ------------------------------------------------------------------------------

// xv[e] of every kept key (0 for NA_KEY); *n_na += the NA_KEY pairs (the caller zeroes it)
__global__ void __launch_bounds__(CT)
k_mantel_xquant(const unsigned long long* __restrict__ kept, long long n, unsigned long long* __restrict__ xv,
                unsigned long long* __restrict__ n_na) {
  __shared__ unsigned int s_na;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_na = 0u;
  __syncthreads();
  unsigned int na = 0u;
  for (long long base = (long long)blockIdx.x * CT; base < n; base += (long long)gridDim.x * CT) {
    const long long e = base + tid;
    const bool in = e < n;
    const unsigned long long key = in ? kept[e] : 0ull;
    na += (unsigned int)__popcll(__ballot(in && key == NA_KEY));
    if (in) xv[e] = key == NA_KEY ? 0ull : mantel::quantise_x(mantel::key_value(key));
  }
  if ((tid & 63) == 0) atomicAdd(&s_na, na);   // the ballots gave every lane the wave's count
  __syncthreads();
  if (tid == 0 && s_na) atomicAdd(n_na, (unsigned long long)s_na);
}

// out[MANTEL_M_*] (zeroed by the caller) += the limbs of v and of v^2 over the plane
__global__ void __launch_bounds__(CT)
k_mantel_moments(const unsigned long long* __restrict__ plane, long long n, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[4];
  const int tid = (int)threadIdx.x;
  unsigned long long s_lo = 0ull, s_hi = 0ull, q_lo = 0ull, q_hi = 0ull;
  for (long long e = (long long)blockIdx.x * CT + tid; e < n; e += (long long)gridDim.x * CT) {
    const unsigned long long v = plane[e] & 0xFFFFFFFFull, q = v * v;
    s_lo += mantel::limb_lo(v);
    s_hi += mantel::limb_hi(v);
    q_lo += mantel::limb_lo(q);
    q_hi += mantel::limb_hi(q);
  }
  s_lo = block_reduce(s_lo, sh, Add());
  s_hi = block_reduce(s_hi, sh, Add());
  q_lo = block_reduce(q_lo, sh, Add());
  q_hi = block_reduce(q_hi, sh, Add());
  if (tid == 0) {
    if (s_lo) atomicAdd(&out[MANTEL_M_S_LO], s_lo);
    if (s_hi) atomicAdd(&out[MANTEL_M_S_HI], s_hi);
    if (q_lo) atomicAdd(&out[MANTEL_M_Q_LO], q_lo);
    if (q_hi) atomicAdd(&out[MANTEL_M_Q_HI], q_hi);
  }
}

// ---- the permutation kernel ----------------------------------------------------------------------------------------

// permT [groups][S][ANO_PB] halfwords: pi_t(s) of ANO_PB permutations side by side per sample (the label plane of
// k_anosim_perm, a permutation being a labelling with S classes), the grid (group of permutations, column strip, run of
// rows), the 256-column chunks, the ANO_PB indices of a thread's column in registers, the row's indices by scalar loads
// and xv read coalesced one row ahead: all k_anosim_perm's (icikt_anosim.hip says why).  What differs is the work per
// row and permutation: one 4-byte gather at tab[pi(i) S + pi(j)] -- the row base is uniform, the 64 columns of a wave
// are scattered over one table row -- a 32 x 32 -> 64 bit product, and its two halves added to two 64-bit sums.
// Threads with j <= i (the rows that cross the diagonal) or j past the strip have xv = 0 and add 0; their gather reads
// a valid word all the same.  At the end: a wave and workgroup reduction and two 64-bit atomicAdds per permutation
// into t_lo / t_hi [groups][ANO_PB] (the caller zeroes them).  No double is ever added.
__global__ void __launch_bounds__(256)
k_mantel_perm(const unsigned long long* __restrict__ xv, const uint32_t* __restrict__ tab, const uint16_t* __restrict__ permT,
              int S, int T, int RR, unsigned long long* __restrict__ t_lo, unsigned long long* __restrict__ t_hi) {
  __shared__ unsigned long long s_lo[4][ANO_PB];
  __shared__ unsigned long long s_hi[4][ANO_PB];
  const int tid = (int)threadIdx.x;
  const int j0 = (int)blockIdx.y * T;
  const int jend = j0 + T < S ? j0 + T : S;
  const int i0 = (int)blockIdx.z * RR;
  const int i1 = i0 + RR < jend - 1 ? i0 + RR : jend - 1;   // rows i <= jend - 2 have a column of the strip
  if (i0 >= i1) return;                                      // (the same for every thread of the workgroup)
  const uint16_t* __restrict__ perm = permT + (size_t)blockIdx.x * (size_t)S * ANO_PB;
  const uint32_t uS = (uint32_t)S;
  unsigned long long acc_lo[ANO_PB], acc_hi[ANO_PB];
#pragma unroll
  for (int p = 0; p < ANO_PB; ++p) { acc_lo[p] = 0ull; acc_hi[p] = 0ull; }
  for (int c0 = j0; c0 < jend; c0 += 256) {
    const int j = c0 + tid;
    const bool col = j < jend;
    if (c0 + 255 <= i0) continue;   // every column of the chunk lies at or below the run's first row
    uint32_t cl[ANO_PB];
    {
      const uint4* q = reinterpret_cast<const uint4*>(perm + (size_t)(col ? j : 0) * ANO_PB);
#pragma unroll
      for (int v = 0; v < ANO_PB / 8; ++v) {
        const uint4 u = q[v];
        cl[8 * v + 0] = u.x & 0xFFFFu; cl[8 * v + 1] = u.x >> 16;
        cl[8 * v + 2] = u.y & 0xFFFFu; cl[8 * v + 3] = u.y >> 16;
        cl[8 * v + 4] = u.z & 0xFFFFu; cl[8 * v + 5] = u.z >> 16;
        cl[8 * v + 6] = u.w & 0xFFFFu; cl[8 * v + 7] = u.w >> 16;
      }
#pragma unroll
      for (int p = 0; p < ANO_PB; ++p) cl[p] = cl[p] < uS ? cl[p] : 0u;   // (the host has checked: never taken)
    }
    const int cend = c0 + 256 < jend ? c0 + 256 : jend;
    const int iend = i1 < cend - 1 ? i1 : cend - 1;          // rows below the chunk's last column
    long long at = (long long)i0 * (2ll * S - i0 - 1) / 2 - i0 - 1 + j;   // the pair (i, j) of row i = i0
    uint32_t ahead = (col && j > i0 && i0 < iend) ? (uint32_t)xv[at] : 0u;   // a row's value is read one row ahead
    for (int i = i0; i < iend; ++i) {
      const uint4* q = reinterpret_cast<const uint4*>(perm + (size_t)i * ANO_PB);   // (uniform: scalar loads)
      const uint32_t x = ahead;
      at += S - i - 2;                                                              // the pair (i + 1, j)
      ahead = (col && j > i + 1 && i + 1 < iend) ? (uint32_t)xv[at] : 0u;
#pragma unroll
      for (int v = 0; v < ANO_PB / 8; ++v) {
        const uint4 u = q[v];
        const uint32_t rl[8] = {u.x & 0xFFFFu, u.x >> 16, u.y & 0xFFFFu, u.y >> 16,
                                u.z & 0xFFFFu, u.z >> 16, u.w & 0xFFFFu, u.w >> 16};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t pi = rl[k] < uS ? rl[k] : 0u;
          const uint32_t y = tab[(size_t)pi * (size_t)uS + (size_t)cl[8 * v + k]];
          const unsigned long long prod = (unsigned long long)x * (unsigned long long)y;
          acc_lo[8 * v + k] += mantel::limb_lo(prod);
          acc_hi[8 * v + k] += mantel::limb_hi(prod);
        }
      }
    }
  }
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int p = 0; p < ANO_PB; ++p) {
    unsigned long long a = acc_lo[p], b = acc_hi[p];
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
    }
    if (lane == 0) { s_lo[w][p] = a; s_hi[w][p] = b; }
  }
  __syncthreads();
  if (tid < ANO_PB) {
    const unsigned long long a = s_lo[0][tid] + s_lo[1][tid] + s_lo[2][tid] + s_lo[3][tid];
    const unsigned long long b = s_hi[0][tid] + s_hi[1][tid] + s_hi[2][tid] + s_hi[3][tid];
    const size_t slot = (size_t)blockIdx.x * ANO_PB + (size_t)tid;
    if (a) atomicAdd(&t_lo[slot], a);
    if (b) atomicAdd(&t_hi[slot], b);
  }
}

unsigned grid_for(long long n, long long cap) {
  const long long want = (n + CT - 1) / CT;
  return (unsigned)(want < cap ? want : cap);
}

}  // namespace

hipError_t launch_mantel_ykeys(unsigned long long* plane, long long n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mantel_ykeys, dim3(grid_for(n, 16384)), dim3(CT), 0, s, plane, n);
  return hipGetLastError();
}

hipError_t launch_mantel_yquant(const unsigned long long* y, long long n, double lo, int ex, unsigned long long* yv,
                                hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (y == yv) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mantel_yquant, dim3(grid_for(n, 16384)), dim3(CT), 0, s, y, n, lo, ex, yv);
  return hipGetLastError();
}

hipError_t launch_mantel_expand(const unsigned long long* plane, int S, uint32_t* tab, hipStream_t s) {
  if (S < 1) return hipSuccess;
  if (S > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mantel_expand, dim3((unsigned)(S < 4096 ? S : 4096)), dim3(CT), 0, s, plane, S, tab);
  return hipGetLastError();
}

hipError_t launch_mantel_xquant(const unsigned long long* kept, long long n, unsigned long long* xv,
                                unsigned long long* n_na, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (kept == xv) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mantel_xquant, dim3(grid_for(n, 2048)), dim3(CT), 0, s, kept, n, xv, n_na);
  return hipGetLastError();
}

hipError_t launch_mantel_moments(const unsigned long long* plane, long long n, unsigned long long* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mantel_moments, dim3(grid_for(n, 2048)), dim3(CT), 0, s, plane, n, out);
  return hipGetLastError();
}

hipError_t launch_mantel_perm(const unsigned long long* xv, const uint32_t* tab, const uint16_t* permT, int S, int n_groups,
                              int strip, unsigned long long* t_lo, unsigned long long* t_hi, hipStream_t s) {
  if (S < 2 || n_groups <= 0) return hipSuccess;
  if (S > 65535 || strip < ANO_STRIP_MIN || strip > ANO_STRIP_MAX) return hipErrorInvalidValue;
  const int n_strips = (S + strip - 1) / strip;
  const int n_runs = (S - 1 + MANTEL_ROW_RUN - 1) / MANTEL_ROW_RUN;
  if (n_strips > 65535 || n_runs > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const dim3 grid((unsigned)n_groups, (unsigned)n_strips, (unsigned)n_runs);
  hipLaunchKernelGGL(k_mantel_perm, grid, dim3(256), 0, s, xv, tab, permT, S, strip, MANTEL_ROW_RUN, t_lo, t_hi);
  return hipGetLastError();
}

}  // namespace icikt
