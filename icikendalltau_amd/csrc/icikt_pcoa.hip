// icikt_pcoa.hip -- principal coordinates (classical scaling; Gower 1966) of the samples under the dissimilarity
// 1 - raw, on the device (icikt_pcoa_f64, host side: icikt_capi_pcoa.cpp).
//
// The rule, the device's half.  A pair's q is PERMANOVA's integer fixed::quantise_key(key) of its kept key
// (icikt_fixed.h), e^ = (double)q 2^-50 its squared dissimilarity (exact: q <= 2^52), e^_ii = 0.  With the row means
// m_i and the grand mean m-bar -- correctly rounded on the host from the integer row sums -- a cell of the centred
// table is  G_ij = -0.5 * ((e^_ij - (m_i + m_j)) + m-bar),  exactly these four operations with contraction off: G is
// symmetric to the bit and the same for every block cut.  What follows is a block Krylov iteration whose every
// floating-point sum has a fixed order: no kernel of this file adds doubles with atomics.
//
//   k_pcoa_rows     one workgroup per sample s, k_disp_table's addressing: the partners t > s are row s of the triangle,
//                   contiguous; the partners t < s are column s, one key per row, strided.  R_s as two limbs, and (row
//                   role only, every pair once) the NA_KEY pairs: one integer atomic per workgroup.
//   k_pcoa_centre   one thread per cell (i, j): the key of the pair, q, e^, G_ij; the diagonal included, every cell
//                   written.
//   k_pcoa_apply    W = G V for an S x b block (b <= 64): the hot kernel, see below.
//   k_pcoa_qtw      C = Q^T W          (L x b)      one workgroup per (basis column, group of 8 block columns)
//   k_pcoa_axz      Out = A Z or Out -= A Z (S x b)  one thread per row and group of 8 columns, l = 0 .. L - 1 in order
//   k_pcoa_sumsq    the sum of squares of every column of a block (norms; applied to G's rows, then to the S row
//                   sums, it is |G|_F^2 in a fixed order)
//   k_pcoa_scale    a column divided by its norm, or zeroed and flagged as dropped when the norm is below the threshold
//   k_pcoa_resid    |GY_c - theta_c Y_c|^2 per Ritz pair
//   k_pcoa_sign     the sign rule: a vector's component of largest magnitude is positive, the smallest index deciding
//                   among equal magnitudes
//
// K_PCOA_APPLY.  A workgroup of 4 waves takes 4 RW consecutive rows of G, a wave RW of them.  The columns j are taken
// in chunks of JT; the chunk of V, JT x CB doubles (32 KB), is staged in LDS column by column, so that lane l reads
// Vs[c][u 64 + l] without a bank conflict, and every wave of the workgroup uses it: V leaves L2 once per workgroup, not
// once per wave.  A lane reads G[i][j0 + u 64 + l] for its RW rows -- 512 contiguous bytes per wave-instruction, RW JT /
// 64 = 16 of them in flight per wave before the first is used -- and keeps RW x CB accumulators (64 doubles for every
// CB: (CB, RW) is (16, 4), (32, 2) or (64, 1)), so G is read once per application whatever b.  A row's sum is taken per
// lane over j ascending and then over the lanes by the xor tree: a fixed order for a given S.  (8-byte lanes, not 16:
// a row of an odd S does not start on a 16-byte boundary.)  Arithmetic against the read, and why the f64 MFMA is not
// used: DESIGN.md section 27.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_fixed.h"

namespace icikt {

namespace {

using namespace colsort;

// first pair of row i of combn(S, 2) (cut_rows' formula, icikt_blocks.h)
__device__ __forceinline__ long long pcoa_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum over the workgroup (CT threads) in a fixed order: the xor tree of each wave, then the waves 0, 1, 2, 3
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(CT)
k_pcoa_rows(const unsigned long long* __restrict__ kept, int S, unsigned long long* __restrict__ row_lo,
            unsigned long long* __restrict__ row_hi, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long sh[4];
  const int tid = (int)threadIdx.x;
  const int s = (int)blockIdx.x;
  if (s >= S) return;                                  // (the same for every thread of the workgroup)
  const long long row_s = pcoa_rowoff(S, s) - s - 1;   // + t: the pair (s, t), t > s
  unsigned long long lo = 0ull, hi = 0ull, na = 0ull;
  for (int t = tid; t < S; t += CT) {
    if (t == s) continue;
    const unsigned long long key = t > s ? kept[row_s + t] : kept[pcoa_rowoff(S, t) + (s - t - 1)];
    if (t > s && key == NA_KEY) na += 1ull;
    const unsigned long long v = fixed::quantise_key(key);
    lo += fixed::limb_lo(v);
    hi += fixed::limb_hi(v);
  }
  lo = block_reduce(lo, sh, Add());                    // integers: the order does not show
  hi = block_reduce(hi, sh, Add());
  na = block_reduce(na, sh, Add());
  if (tid == 0) {
    row_lo[s] = lo;
    row_hi[s] = hi;
    if (na) atomicAdd(&totals[PMV_T_NA], na);
  }
}

__global__ void __launch_bounds__(CT)
k_pcoa_centre(const unsigned long long* __restrict__ kept, const double* __restrict__ mean, const double* __restrict__ grand,
              int S, double* __restrict__ G) {
#pragma clang fp contract(off)
  const int i = (int)blockIdx.y;
  const int j = (int)(blockIdx.x * CT + threadIdx.x);
  if (i >= S || j >= S) return;
  double e = 0.0;
  if (i != j) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    e = ldexp((double)fixed::quantise_key(kept[pcoa_rowoff(S, lo) + (hi - lo - 1)]), -fixed::FRAC_BITS);
  }
  const double mm = mean[i] + mean[j];
  const double t = e - mm;
  const double u = t + grand[0];
  G[(long long)i * S + j] = -0.5 * u;
}

constexpr int APPLY_LDS_DOUBLES = 4096;   // JT x CB: 32 KB

template <int CB, int RW>
__global__ void __launch_bounds__(CT)
k_pcoa_apply(const double* __restrict__ G, const double* __restrict__ V, int S, int b, double* __restrict__ W) {
  constexpr int JT = APPLY_LDS_DOUBLES / CB;   // columns of G per chunk
  constexpr int U = JT / 64;                   // ... per lane
  __shared__ double Vs[CB][JT];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = ((int)blockIdx.x * 4 + wave) * RW;   // the wave's first row
  double acc[RW][CB];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[r][c] = 0.0;
  for (int j0 = 0; j0 < S; j0 += JT) {
    __syncthreads();                                   // the chunk before has been used by every wave
    for (int idx = tid; idx < CB * JT; idx += CT) {
      const int c = idx / JT, jj = idx % JT;
      Vs[c][jj] = (c < b && j0 + jj < S) ? V[(long long)c * S + j0 + jj] : 0.0;
    }
    __syncthreads();
    double g[RW][U];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u * 64 + lane;
        g[r][u] = (i0 + r < S && j < S) ? G[(long long)(i0 + r) * S + j] : 0.0;
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const double v = Vs[c][u * 64 + lane];
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r][c] += g[r][u] * v;
      }
  }
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const double v = wave_sum_f64(acc[r][c]);
      if (lane == 0 && i0 + r < S && c < b) W[(long long)c * S + i0 + r] = v;
    }
}

constexpr int COLS = 8;   // block columns a thread or workgroup of the skinny kernels takes at once

// C[l + ldc c] = sum_i Q[i + S l] W[i + S c], l = blockIdx.x < L, c in the group blockIdx.y of COLS columns below b
__global__ void __launch_bounds__(CT)
k_pcoa_qtw(const double* __restrict__ Q, const double* __restrict__ W, int S, int b, int ldc, double* __restrict__ C) {
  __shared__ double sh[4];
  const int l = (int)blockIdx.x, c0 = (int)blockIdx.y * COLS;
  const double* q = Q + (long long)l * S;
  double acc[COLS];
#pragma unroll
  for (int c = 0; c < COLS; ++c) acc[c] = 0.0;
  for (int i = (int)threadIdx.x; i < S; i += CT) {
    const double qv = q[i];
#pragma unroll
    for (int c = 0; c < COLS; ++c)
      if (c0 + c < b) acc[c] += qv * W[(long long)(c0 + c) * S + i];
  }
#pragma unroll
  for (int c = 0; c < COLS; ++c) {
    const double v = block_sum_f64(acc[c], sh);
    if (threadIdx.x == 0 && c0 + c < b) C[l + (long long)ldc * (c0 + c)] = v;
  }
}

// Out[i + S c] (-)= sum_l A[i + S l] Z[l + ldz c], l ascending; c in the group blockIdx.y of COLS columns below b
template <bool SUB>
__global__ void __launch_bounds__(CT)
k_pcoa_axz(const double* __restrict__ A, const double* __restrict__ Z, int S, int L, int b, int ldz, double* __restrict__ Out) {
  const int i = (int)(blockIdx.x * CT + threadIdx.x), c0 = (int)blockIdx.y * COLS;
  if (i >= S) return;
  double acc[COLS];
#pragma unroll
  for (int c = 0; c < COLS; ++c) acc[c] = 0.0;
  for (int l = 0; l < L; ++l) {
    const double a = A[(long long)l * S + i];
#pragma unroll
    for (int c = 0; c < COLS; ++c)
      if (c0 + c < b) acc[c] += a * Z[l + (long long)ldz * (c0 + c)];
  }
#pragma unroll
  for (int c = 0; c < COLS; ++c)
    if (c0 + c < b) {
      double* o = Out + (long long)(c0 + c) * S + i;
      *o = SUB ? *o - acc[c] : acc[c];
    }
}

// out[c] = sum_i X[i + ld c]^2, c = blockIdx.x
__global__ void __launch_bounds__(CT)
k_pcoa_sumsq(const double* __restrict__ X, int n, long long ld, double* __restrict__ out) {
  __shared__ double sh[4];
  const double* x = X + (long long)blockIdx.x * ld;
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += CT) acc += x[i] * x[i];
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// out[0] = sum_i x[i] in a fixed order (one workgroup)
__global__ void __launch_bounds__(CT)
k_pcoa_sum(const double* __restrict__ x, int n, double* __restrict__ out) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += CT) acc += x[i];
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) out[0] = acc;
}

// the column x [n] with the sum of squares sumsq[0]: below thr2 it is zeroed and flag[0] = 0, else divided by its norm
// and flag[0] = 1
__global__ void __launch_bounds__(CT)
k_pcoa_scale(double* __restrict__ x, int n, const double* __restrict__ sumsq, double thr2, int32_t* __restrict__ flag) {
  const int i = (int)(blockIdx.x * CT + threadIdx.x);
  const double ss = sumsq[0];
  const bool keep = ss >= thr2 && ss > 0.0;
  if (i == 0) flag[0] = keep ? 1 : 0;
  if (i >= n) return;
  x[i] = keep ? x[i] / sqrt(ss) : 0.0;
}

// out[c] = sum_i (GY[i + S c] - theta[c] Y[i + S c])^2, c = blockIdx.x
__global__ void __launch_bounds__(CT)
k_pcoa_resid(const double* __restrict__ GY, const double* __restrict__ Y, const double* __restrict__ theta, int S,
             double* __restrict__ out) {
  __shared__ double sh[4];
  const long long off = (long long)blockIdx.x * S;
  const double th = theta[blockIdx.x];
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < S; i += CT) {
    const double r = GY[off + i] - th * Y[off + i];
    acc += r * r;
  }
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// column c = blockIdx.x of Y [S]: the component of largest magnitude, the smallest index among equals, made positive
__global__ void __launch_bounds__(CT)
k_pcoa_sign(double* __restrict__ Y, int S) {
  __shared__ double s_mag[CT];
  __shared__ int s_idx[CT];
  double* y = Y + (long long)blockIdx.x * S;
  const int tid = (int)threadIdx.x;
  double mag = -1.0;
  int idx = S;
  for (int i = tid; i < S; i += CT) {                  // (i ascending: a later equal magnitude does not replace)
    const double a = fabs(y[i]);
    if (a > mag) { mag = a; idx = i; }
  }
  s_mag[tid] = mag;
  s_idx[tid] = idx;
  __syncthreads();
  for (int o = CT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double m2 = s_mag[tid + o];
      const int i2 = s_idx[tid + o];
      if (m2 > s_mag[tid] || (m2 == s_mag[tid] && i2 < s_idx[tid])) { s_mag[tid] = m2; s_idx[tid] = i2; }
    }
    __syncthreads();
  }
  const int best = s_idx[0];
  if (best >= S) return;                               // (the same for every thread: an empty or all-NaN column)
  const bool flip = y[best] < 0.0;
  __syncthreads();                                     // every thread has read y[best] before anyone writes it
  if (flip)
    for (int i = tid; i < S; i += CT) y[i] = -y[i];
}

inline bool pcoa_shape_ok(int S) { return S >= 1 && S <= 65535; }

}  // namespace

hipError_t launch_pcoa_rows(const unsigned long long* kept, int S, unsigned long long* row_lo, unsigned long long* row_hi,
                            unsigned long long* totals, hipStream_t s) {
  if (!pcoa_shape_ok(S)) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_rows, dim3((unsigned)S), dim3(CT), 0, s, kept, S, row_lo, row_hi, totals);
  return hipGetLastError();
}

hipError_t launch_pcoa_centre(const unsigned long long* kept, const double* mean, const double* grand, int S, double* G,
                              hipStream_t s) {
  if (!pcoa_shape_ok(S)) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_centre, dim3((unsigned)((S + CT - 1) / CT), (unsigned)S), dim3(CT), 0, s, kept, mean, grand, S, G);
  return hipGetLastError();
}

hipError_t launch_pcoa_apply(const double* G, const double* V, int S, int b, double* W, hipStream_t s) {
  if (!pcoa_shape_ok(S) || b < 1 || b > PCOA_MAX_BLOCK) return hipErrorInvalidValue;
  (void)hipGetLastError();
  if (b <= 16)
    hipLaunchKernelGGL((k_pcoa_apply<16, 4>), dim3((unsigned)((S + 15) / 16)), dim3(CT), 0, s, G, V, S, b, W);
  else if (b <= 32)
    hipLaunchKernelGGL((k_pcoa_apply<32, 2>), dim3((unsigned)((S + 7) / 8)), dim3(CT), 0, s, G, V, S, b, W);
  else
    hipLaunchKernelGGL((k_pcoa_apply<64, 1>), dim3((unsigned)((S + 3) / 4)), dim3(CT), 0, s, G, V, S, b, W);
  return hipGetLastError();
}

hipError_t launch_pcoa_qtw(const double* Q, int L, const double* W, int S, int b, int ldc, double* C, hipStream_t s) {
  if (L <= 0 || b <= 0) return hipSuccess;
  if (!pcoa_shape_ok(S) || L > 65535 || b > 65535 || ldc < L) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_qtw, dim3((unsigned)L, (unsigned)((b + COLS - 1) / COLS)), dim3(CT), 0, s, Q, W, S, b, ldc, C);
  return hipGetLastError();
}

hipError_t launch_pcoa_axz(const double* A, int L, const double* Z, int ldz, int S, int b, int subtract, double* Out,
                           hipStream_t s) {
  if (b <= 0 || (subtract && L <= 0)) return hipSuccess;
  if (!pcoa_shape_ok(S) || L < 0 || b > 65535 || ldz < L) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const dim3 grid((unsigned)((S + CT - 1) / CT), (unsigned)((b + COLS - 1) / COLS));
  if (subtract) hipLaunchKernelGGL(k_pcoa_axz<true>, grid, dim3(CT), 0, s, A, Z, S, L, b, ldz, Out);
  else hipLaunchKernelGGL(k_pcoa_axz<false>, grid, dim3(CT), 0, s, A, Z, S, L, b, ldz, Out);
  return hipGetLastError();
}

hipError_t launch_pcoa_sumsq(const double* X, int n, long long ld, int cols, double* out, hipStream_t s) {
  if (cols <= 0) return hipSuccess;
  if (n < 0 || n > 65535 || cols > 65535 || ld < n) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_sumsq, dim3((unsigned)cols), dim3(CT), 0, s, X, n, ld, out);
  return hipGetLastError();
}

hipError_t launch_pcoa_sum(const double* x, int n, double* out, hipStream_t s) {
  if (n < 0 || n > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_sum, dim3(1), dim3(CT), 0, s, x, n, out);
  return hipGetLastError();
}

hipError_t launch_pcoa_scale(double* x, int n, const double* sumsq, double thr2, int32_t* flag, hipStream_t s) {
  if (n < 1 || n > 65535) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_scale, dim3((unsigned)((n + CT - 1) / CT)), dim3(CT), 0, s, x, n, sumsq, thr2, flag);
  return hipGetLastError();
}

hipError_t launch_pcoa_resid(const double* GY, const double* Y, const double* theta, int S, int k, double* out,
                             hipStream_t s) {
  if (k <= 0) return hipSuccess;
  if (!pcoa_shape_ok(S) || k > PCOA_MAX_BLOCK) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_resid, dim3((unsigned)k), dim3(CT), 0, s, GY, Y, theta, S, out);
  return hipGetLastError();
}

hipError_t launch_pcoa_sign(double* Y, int S, int k, hipStream_t s) {
  if (k <= 0) return hipSuccess;
  if (!pcoa_shape_ok(S) || k > PCOA_MAX_BLOCK) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_pcoa_sign, dim3((unsigned)k), dim3(CT), 0, s, Y, S);
  return hipGetLastError();
}

}  // namespace icikt
