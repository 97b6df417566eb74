// icikt_cor.hip -- cor_fast (R/other_correlations.R): Pearson / Spearman estimates and cor.test p-values for a pair list.
//
//   KC0  k_cor_prep          one workgroup per column: non-NA count, Pearson: column shifted by its own mean and scaled
//                            by a power of two (NA = NaN), Σz, Σz², Spearman: doubled average ranks
//                            (rank(ties.method = "average") * 2, integers) centred on n + 1, the sorted order and each
//                            sorted position's tie-group bounds
//   KC1  k_cor_tile          all pairs (+ self pairs) without NA: one 64 x 64 tile of Z^T Z per workgroup (f64 FMA)
//        k_cor_dots          any pair list: one wave per pair; dense (Z^T Z) or pairwise Pearson (two passes over the
//                            raw columns: the jointly present rows' n, mean, min / max, then their centred sums)
//        k_cor_spearman_pw   pairwise Spearman with NA: one workgroup per pair, O(n), no per-pair sort: the subset ranks
//                            of each side from prefix counts of the other side's presence along its sorted order
//   KC2  k_cor_epilogue      one thread per pair: rho, stats::cor.test.default's p-value, n_values, reason
// DESIGN.md section 9 restates the formulas and names their sources.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {
namespace {

using namespace colsort;

template <typename T>
__device__ inline T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// TwoSum (Knuth): hi + lo += v with the rounding error of hi + v kept exactly in lo
__device__ inline void two_sum_acc(double& hi, double& lo, double v) {
  const double s = hi + v, bp = s - hi;
  lo += (hi - (s - bp)) + (v - bp);
  hi = s;
}

// the wave's TwoSum total; (lo + l) + err is symmetric in the two lanes of a step, so every lane ends with the same
// hi and lo
__device__ inline void wave_two_sum(double& hi, double& lo) {
  for (int o = 32; o > 0; o >>= 1) {
    const double h = __shfl_xor(hi, o, 64), l = __shfl_xor(lo, o, 64);
    const double s = hi + h, bp = s - hi;
    lo = (lo + l) + ((hi - (s - bp)) + (h - bp));
    hi = s;
  }
}

// 2^-e for the spread s in [2^(e-1), 2^e): an exact rescaling of deviations up to s into [0.5, 1), so that their
// squares neither overflow (s ~ 1e300) nor underflow (s ~ 1e-300); 1 when s is 0, Inf or NaN
__device__ inline double cor_scale(double s) {
  if (!(s > 0.0) || s - s != 0.0) return 1.0;
  int e;
  frexp(s, &e);
  return ldexp(1.0, -(e < -1022 ? -1022 : e));
}

__global__ void __launch_bounds__(CT) k_cor_prep(CorPrep cp) {
  __shared__ double shd[4];
  __shared__ int shi[4];
  __shared__ long long shl[4];
  __shared__ uint64_t sk[SORT_TILE];
  __shared__ int32_t si[SORT_TILE];
  const int64_t n = cp.n;
  for (int c = blockIdx.x; c < cp.S; c += gridDim.x) {
    const double* x = cp.X + (int64_t)c * cp.ld;
    double* z = cp.Z + (int64_t)c * n;
    int cnt = 0, cntf = 0;
    double sum = 0.0, mn = INFINITY, mx = -INFINITY, mnf = INFINITY, mxf = -INFINITY;
    for (int64_t r = threadIdx.x; r < n; r += CT) {
      const double v = x[r];
      if (v == v) {
        ++cnt;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
        if (v - v == 0.0) { ++cntf; sum += v; mnf = fmin(mnf, v); mxf = fmax(mxf, v); }
      }
    }
    cnt = block_reduce(cnt, shi, Add());
    cntf = block_reduce(cntf, shi, Add());
    sum = block_reduce(sum, shd, Add());
    mn = block_reduce(mn, shd, Min());
    mx = block_reduce(mx, shd, Max());
    mnf = block_reduce(mnf, shd, Min());
    mxf = block_reduce(mxf, shd, Max());
    uint32_t fl = (cnt == 0 || mn == mx) ? COR_CONSTANT : 0u;
    if (cp.method == 0) {
      // Pearson: shift by the mean of the finite values, refined once (a constant column becomes exactly 0)
      double m1 = cntf ? sum / cntf : 0.0, corr = 0.0;
      for (int64_t r = threadIdx.x; r < n; r += CT) {
        const double v = x[r];
        if (v - v == 0.0) corr += v - m1;
      }
      corr = block_reduce(corr, shd, Add());
      const double mean = cntf ? m1 + corr / cntf : 0.0;
      // Z = (x - mean) 2^-e, the largest finite deviation in [0.5, 1); Σz and Σz² of the same Z: the products kernels
      // subtract Σz_i Σz_j / n, which takes out the rounding of the mean (n δ², large when |mean| >> sd)
      const double sc = cntf ? cor_scale(fmax(mxf - mean, mean - mnf)) : 1.0;
      double ss = 0.0, sz = 0.0;
      for (int64_t r = threadIdx.x; r < n; r += CT) {
        const double v = x[r];
        const double d = (v == v) ? (v - mean) * sc : (double)NAN;
        z[r] = d;
        if (v == v) { sz += d; ss += d * d; }
      }
      ss = block_reduce(ss, shd, Add());
      sz = block_reduce(sz, shd, Add());
      if (threadIdx.x == 0) {
        cp.cnt[c] = cnt;
        cp.colss[c] = cnt ? ss - sz * sz / cnt : 0.0;
        cp.colsum[c] = sz;
        cp.flags[c] = fl;
      }
      continue;
    }
    // Spearman: sort, tie groups, doubled average ranks
    uint64_t* keys = cp.keys + (int64_t)blockIdx.x * cp.np2;
    int32_t* idx = cp.idx + (int64_t)blockIdx.x * cp.np2;
    for (int r = threadIdx.x; r < cp.np2; r += CT) {
      keys[r] = r < n ? cor_key(x[r]) : NA_KEY;
      idx[r] = r < n ? r : -1;
    }
    __syncthreads();
    block_sort(keys, idx, cp.np2, sk, si);
    int32_t* ord = cp.ord + (int64_t)c * n;
    int32_t* gs = cp.gs + (int64_t)c * n;
    int32_t* ge = cp.ge + (int64_t)c * n;
    long long ss = 0;
    int tied = 0;
    tie_groups(keys, cnt, gs, shi, [&](int p, int g0, int g1) {
      ge[p] = g1;
      ord[p] = idx[p];
      const long long r2 = (long long)g0 + g1 - cnt;   // 2 * rank - (cnt + 1)
      z[idx[p]] = (double)r2;
      ss += r2 * r2;
      tied |= (g1 - g0 >= 2);
    });
    for (int p = cnt + threadIdx.x; p < cp.np2; p += CT)   // NA rows and the padding (row -1) share the last key
      if (idx[p] >= 0) z[idx[p]] = (double)NAN;
    ss = block_reduce(ss, shl, Add());
    tied = block_reduce(tied, shi, Max());
    if (tied) fl |= COR_TIES;
    if (threadIdx.x == 0) { cp.cnt[c] = cnt; cp.colss[c] = (double)ss; cp.colsum[c] = 0.0; cp.flags[c] = fl; }
    __syncthreads();
  }
}

// pair index of (i, j), i <= j, in combn(S, 2) order followed by the S self pairs (diag: none when false)
__device__ inline int64_t combn_index(int64_t i, int64_t j, int64_t S) {
  return i * S - i * (i + 1) / 2 + (j - i - 1);
}

// colss holds the corrected Σz² - (Σz)² / n, so a self pair is the very sum of its variances: rho = 1 exactly
__device__ inline void dense_acc(CorAcc* a, double sxy, int i, int j, const int32_t* cnt, const double* colss,
                                 const double* colsum, const uint8_t* flags) {
  a->m = (double)cnt[i];
  a->sxy = (i == j) ? colss[i] : sxy - colsum[i] * colsum[j] / a->m;
  a->sxx = colss[i];
  a->syy = colss[j];
  a->flags = (uint32_t)flags[i] | ((uint32_t)flags[j] << 8);
}

// Z^T Z over the upper triangle of 64 x 64 tiles; thread (ty, tx) holds rows ty + 16 a, columns tx + 16 b of its tile
__global__ void __launch_bounds__(CT) k_cor_tile(const double* __restrict__ Z, int64_t n, int S, int diag,
                                                 const int32_t* __restrict__ cnt, const double* __restrict__ colss,
                                                 const double* __restrict__ colsum, const uint8_t* __restrict__ flags,
                                                 CorAcc* __restrict__ acc) {
  constexpr int T = 64, KB = 16;
  __shared__ double A[KB][T + 1], B[KB][T + 1];
  // blockIdx.x -> (bi, bj), bi <= bj
  const int nb = (S + T - 1) / T;
  int64_t t = blockIdx.x;
  int bi = 0;
  while (t >= nb - bi) { t -= nb - bi; ++bi; }
  const int bj = bi + (int)t;
  const int i0 = bi * T, j0 = bj * T;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double s[4][4] = {};
  for (int64_t k0 = 0; k0 < n; k0 += KB) {
    for (int e = threadIdx.x; e < KB * T; e += CT) {
      const int kk = e % KB, cc = e / KB;   // consecutive threads read consecutive rows of a column
      const int64_t r = k0 + kk;
      A[kk][cc] = (r < n && i0 + cc < S) ? Z[(int64_t)(i0 + cc) * n + r] : 0.0;
      B[kk][cc] = (r < n && j0 + cc < S) ? Z[(int64_t)(j0 + cc) * n + r] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KB; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = A[kk][ty + 16 * u]; b[u] = B[kk][tx + 16 * u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) s[u][v] = fma(a[u], b[v], s[u][v]);
    }
    __syncthreads();
  }
  const int64_t ncombn = (int64_t)S * (S - 1) / 2;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i >= S || j >= S || i > j) continue;
      if (i == j && !diag) continue;
      const int64_t p = (i == j) ? ncombn + i : combn_index(i, j, S);
      dense_acc(&acc[p], s[u][v], i, j, cnt, colss, colsum, flags);
    }
}

// one wave per pair of any list.  Dense: V = Z (stride n), Σ z_i z_j.  PW, pairwise Pearson: V = the raw matrix
// (stride ld, NaN = NA), two passes over the jointly present rows.  Centring on each column's mean (Z) would not do:
// a pair's rows can sit far from it (left-censoring), and the shift has already rounded away what tells them apart.
//   1. count, TwoSum Σx and Σy (means good to an ulp), min / max of the raw values (exact zero-variance test)
//   2. d = (x - mean_x) 2^-ex, e likewise, with 2^-ex from the pair's own spread: Sxy = Σde - Σd Σe / m, and so on
template <bool PW>
__global__ void __launch_bounds__(CT) k_cor_dots(const double* __restrict__ V, int64_t n, int64_t ld,
                                                 const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
                                                 int64_t P, const int32_t* __restrict__ cnt,
                                                 const double* __restrict__ colss, const double* __restrict__ colsum,
                                                 const uint8_t* __restrict__ flags, CorAcc* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (CT / 64);
  for (int64_t p = (int64_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6); p < P; p += nw) {
    const int i = pi[p], j = pj[p];
    const double* x = V + (int64_t)i * ld;
    const double* y = V + (int64_t)j * ld;
    if (!PW) {
      double s = 0.0;
      for (int64_t r = lane; r < n; r += 64) s = fma(x[r], y[r], s);
      s = wave_sum(s);
      if (lane == 0) dense_acc(&acc[p], s, i, j, cnt, colss, colsum, flags);
      continue;
    }
    double m = 0, sx = 0, ex = 0, sy = 0, ey = 0;
    double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
    for (int64_t r = lane; r < n; r += 64) {
      const double a = x[r], b = y[r];
      if (a == a && b == b) {   // (a row with +-Inf on one side and NA on the other stays out)
        m += 1.0;
        two_sum_acc(sx, ex, a);
        two_sum_acc(sy, ey, b);
        mnx = fmin(mnx, a); mxx = fmax(mxx, a); mny = fmin(mny, b); mxy = fmax(mxy, b);
      }
    }
    m = wave_sum(m);
    wave_two_sum(sx, ex);
    wave_two_sum(sy, ey);
    for (int o = 32; o > 0; o >>= 1) {
      mnx = fmin(mnx, __shfl_xor(mnx, o, 64)); mxx = fmax(mxx, __shfl_xor(mxx, o, 64));
      mny = fmin(mny, __shfl_xor(mny, o, 64)); mxy = fmax(mxy, __shfl_xor(mxy, o, 64));
    }
    // (+-Inf in the subset makes the means NaN, then every sum: the epilogue's NA)
    const double mx = m > 0 ? (sx + ex) / m : 0.0, my = m > 0 ? (sy + ey) / m : 0.0;
    const double cx = cor_scale(fmax(mxx - mx, mx - mnx)), cy = cor_scale(fmax(mxy - my, my - mny));
    double sd = 0, se = 0, sdd = 0, see = 0, sde = 0;
    for (int64_t r = lane; r < n; r += 64) {
      const double a = x[r], b = y[r];
      if (a == a && b == b) {
        const double d = (a - mx) * cx, e = (b - my) * cy;
        sd += d; se += e;
        sdd = fma(d, d, sdd); see = fma(e, e, see); sde = fma(d, e, sde);
      }
    }
    sd = wave_sum(sd); se = wave_sum(se);
    sdd = wave_sum(sdd); see = wave_sum(see); sde = wave_sum(sde);
    if (lane == 0) {
      CorAcc a;
      a.m = m;
      if (m > 0) {
        a.sxy = sde - sd * se / m;
        a.sxx = sdd - sd * sd / m;
        a.syy = see - se * se / m;
      } else {
        a.sxy = a.sxx = a.syy = 0.0;
      }
      a.flags = (mnx == mxx ? COR_CONSTANT : 0u) | ((mny == mxy ? COR_CONSTANT : 0u) << 8);
      acc[p] = a;
    }
  }
}

// pairwise Spearman: one workgroup per pair, scratch of 2 n + 1 int32 per workgroup (prefix counts, rank of x by row)
__global__ void __launch_bounds__(CT) k_cor_spearman_pw(CorPrep cp, const int32_t* __restrict__ pi,
                                                        const int32_t* __restrict__ pj, int64_t P, int32_t* scratch,
                                                        CorAcc* __restrict__ acc) {
  __shared__ int shi[4];
  __shared__ long long shl[4];
  const int64_t n = cp.n;
  int32_t* C = scratch + (int64_t)blockIdx.x * (2 * n + 1);
  int32_t* rx = C + n + 1;
  for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
    const int col[2] = {pi[p], pj[p]};
    long long sxy = 0, sq[2] = {0, 0};
    int tied[2] = {0, 0}, m = 0;
    for (int side = 0; side < 2; ++side) {
      const int a = col[side], b = col[1 - side];
      const int na = cp.cnt[a];
      const int32_t* ord = cp.ord + (int64_t)a * n;
      const int32_t* gs = cp.gs + (int64_t)a * n;
      const int32_t* ge = cp.ge + (int64_t)a * n;
      const double* zb = cp.Z + (int64_t)b * n;
      // C[q] = rows of a's sorted positions < q that b also has
      int carry = 0;
      for (int b0 = 0; b0 < na; b0 += CT) {
        const int q = b0 + threadIdx.x;
        const int f = (q < na) ? (zb[ord[q]] == zb[ord[q]]) : 0;
        const int incl = block_scan(f, shi, Add(), 0);
        if (q < na) C[q] = carry + incl - f;
        if (threadIdx.x == CT - 1) shi[0] = carry + incl;
        __syncthreads();
        carry = shi[0];
        __syncthreads();
      }
      if (threadIdx.x == 0) C[na] = carry;
      m = carry;
      __syncthreads();
      // doubled subset rank of each joint row: C[gs] + C[ge] + 1, centred on m + 1
      long long s2 = 0, sp = 0;
      int t = 0;
      for (int q = threadIdx.x; q < na; q += CT) {
        const int row = ord[q];
        if (zb[row] == zb[row]) {
          const int c0 = C[gs[q]], c1 = C[ge[q]];
          const long long r = (long long)c0 + c1 - m;
          s2 += r * r;
          t |= (c1 - c0 >= 2);
          if (side == 0) rx[row] = (int32_t)r;
          else sp += r * (long long)rx[row];
        }
      }
      sq[side] = block_reduce(s2, shl, Add());
      tied[side] = block_reduce(t, shi, Max());
      if (side == 1) sxy = block_reduce(sp, shl, Add());
      __syncthreads();   // C is rebuilt by the other side / the next pair
    }
    if (threadIdx.x == 0) {
      CorAcc a;
      a.m = (double)m;
      a.sxy = (double)sxy;
      a.sxx = (double)sq[0];
      a.syy = (double)sq[1];
      a.flags = (sq[0] == 0 ? COR_CONSTANT : 0u) | (tied[0] ? COR_TIES : 0u) |
                ((sq[1] == 0 ? COR_CONSTANT : 0u) << 8) | ((tied[1] ? COR_TIES : 0u) << 8);
      acc[p] = a;
    }
  }
}

// ---- stats::cor.test.default p-values ------------------------------------------------------------------------------

// lgammacor(x) = lgamma(x) - ((x - 0.5) log x - x + log sqrt(2 pi)), x >= 10 (Stirling series)
__device__ inline double lgammacor(double x) {
  const double r = 1.0 / x, r2 = r * r;
  return r * (1.0 / 12 + r2 * (-1.0 / 360 + r2 * (1.0 / 1260 + r2 * (-1.0 / 1680 + r2 * (1.0 / 1188 + r2 * (-691.0 / 360360))))));
}

// log B(a, b) without the cancellation of lgamma differences at large arguments (R's lbeta)
__device__ inline double cor_lbeta(double a, double b) {
  const double p = fmin(a, b), q = fmax(a, b);
  if (p >= 10.0) {
    const double corr = lgammacor(p) + lgammacor(q) - lgammacor(p + q);
    return -0.5 * log(q) + 0.918938533204672741780329736406 + corr + (p - 0.5) * log(p / (p + q)) + q * log1p(-p / (p + q));
  }
  if (q >= 10.0) {
    const double corr = lgammacor(q) - lgammacor(p + q);
    return lgamma(p) + corr + p - p * log(p + q) + (q - 0.5) * log1p(-p / (p + q));
  }
  return lgamma(p) + lgamma(q) - lgamma(p + q);
}

// I_x(a, b) by its continued fraction (modified Lentz), for x <= (a + 1) / (a + b + 2); y = 1 - x
__device__ inline double incbeta_cf(double a, double b, double x, double y) {
  const double tiny = 1e-300, eps = 1e-16;
  const double front = exp(a * log(x) + b * log(y) - cor_lbeta(a, b)) / a;
  double f = 1.0, c = 1.0, d = 1.0 - (a + b) * x / (a + 1.0);
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  f = d;
  for (int m = 1; m < 200000; ++m) {
    double num = m * (b - m) * x / ((a + 2.0 * m - 1.0) * (a + 2.0 * m));
    d = 1.0 + num * d; if (fabs(d) < tiny) d = tiny;
    c = 1.0 + num / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    f *= d * c;
    num = -(a + m) * (a + b + m) * x / ((a + 2.0 * m) * (a + 2.0 * m + 1.0));
    d = 1.0 + num * d; if (fabs(d) < tiny) d = tiny;
    c = 1.0 + num / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    f *= del;
    if (fabs(del - 1.0) < eps) break;
  }
  return front * f;
}

// the regularized incomplete beta I_x(a, b), y = 1 - x given separately (no cancellation near x = 1)
__device__ inline double incbeta(double a, double b, double x, double y) {
  if (x <= 0.0) return 0.0;
  if (y <= 0.0) return 1.0;
  if (x > (a + 1.0) / (a + b + 2.0)) return 1.0 - incbeta_cf(b, a, y, x);
  return incbeta_cf(a, b, x, y);
}

// P(T > |t|) of Student's t with df degrees of freedom
__device__ inline double t_tail(double t, double df) {
  if (isinf(t)) return 0.0;
  const double t2 = t * t;
  return 0.5 * incbeta(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2));
}

// pt(t, df, lower.tail)
__device__ inline double cor_pt(double t, double df, bool lower) {
  if (t != t || !(df > 0.0)) return (double)NAN;
  const double tail = t_tail(t, df);
  return (lower == (t < 0.0)) ? tail : 1.0 - tail;
}

__device__ inline double pnorm_upper(double x) { return 0.5 * erfc(x * 0.70710678118654752440); }

// prho (AS 89): P[S >= is] (lower = false) or P[S < is] (lower = true), S = sum (rank x - rank y)^2 of n untied rows.
// n <= 9: exact, from upper[] = the permutations with S >= 2 k, k = 0 .. (n^3 - n) / 6, table by table for n = 2 .. 9
__device__ double prho(double is, int n, bool lower, const uint32_t* upper) {
  double pv = lower ? 0.0 : 1.0;
  if (n <= 1 || is <= 0.0) return pv;
  const double n3 = (double)n * ((double)n * n - 1) / 3;
  if (is > n3) return 1.0 - pv;
  if (n <= 9) {
    int off = 0;
    for (int k = 2; k < n; ++k) off += (k * k * k - k) / 6 + 1;
    double fact = 1.0;
    for (int k = 2; k <= n; ++k) fact *= k;
    const int kk = (int)ceil(is / 2.0);
    const double ifr = (double)upper[off + kk];
    return (lower ? fact - ifr : ifr) / fact;
  }
  const double b = 1.0 / n;
  const double x = (6.0 * (is - 1) * b / ((double)n * n - 1) - 1) * sqrt(1 / b - 1);
  double y = x * x;
  const double u = x * b * (0.2274 + b * (0.2531 + 0.1745 * b) +
                            y * (-0.0758 + b * (0.1033 + 0.3932 * b) -
                                 y * b * (0.0879 + 0.0151 * b - y * (0.0072 - 0.0831 * b + y * b * (0.0131 - 4.6e-4 * y)))));
  y = u / exp(y / 2);
  pv = lower ? (1.0 - pnorm_upper(x)) - y : y + pnorm_upper(x);
  return pv < 0 ? 0.0 : (pv > 1 ? 1.0 : pv);
}

__device__ double pspearman(double q, int n, bool lower, bool exact, bool continuity, const uint32_t* upper) {
  if (n <= 1290 && exact) return prho(rint(q) + 2.0 * lower, n, lower, upper);
  const double den = (double)n * ((double)n * n - 1) / 6;
  double r = 1 - q / den;
  if (continuity) r -= (r > 0 ? 1.0 : (r < 0 ? -1.0 : 0.0)) / den;
  return cor_pt(r / sqrt((1 - r * r) / (n - 2)), (double)(n - 2), !lower);
}

__global__ void __launch_bounds__(CT) k_cor_epilogue(const CorAcc* __restrict__ acc, int64_t P, int method, int pairwise,
                                                     int alternative, int continuity, const uint32_t* __restrict__ upper,
                                                     double* __restrict__ out3, int32_t* __restrict__ reasons) {
  const int64_t p = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (p >= P) return;
  const CorAcc a = acc[p];
  const int n = (int)a.m;
  double rho = (double)NAN, pv = (double)NAN;
  int reason = COR_OK;
  const int need = (pairwise || method == 0) ? 3 : 2;   // cor_split: < 3 joint rows; cor.test: < 3 (Pearson) / < 2 finite
  if (n < need) {
    reason = COR_SHORT;
  } else if ((a.flags & COR_CONSTANT) || ((a.flags >> 8) & COR_CONSTANT) || !(a.sxx > 0.0) || !(a.syy > 0.0)) {
    reason = COR_NA;   // zero variance (cor: "the standard deviation is zero"), or +-Inf in a Pearson subset
  } else {
    rho = a.sxy / sqrt(a.sxx * a.syy);
    if (rho != rho) {
      reason = COR_NA;
    } else {
      rho = fmin(1.0, fmax(-1.0, rho));
      if (method == 0) {
        const double df = n - 2;
        const double t = sqrt(df) * rho / sqrt(1 - rho * rho);
        if (alternative == 0) pv = 2.0 * t_tail(t, df);   // the smaller tail itself, never 1 - p
        else pv = cor_pt(t, df, alternative == 1);
      } else {
        const bool ties = ((a.flags | (a.flags >> 8)) & COR_TIES) != 0;
        const bool exact = n < 1290 && !ties;
        if (ties && n < 1290) reason = COR_TIES_WARN;
        const double nn = (double)n;
        const double q = (nn * nn * nn - nn) * (1 - rho) / 6;
        if (alternative == 0) {
          const double ph = (q > (nn * nn * nn - nn) / 6) ? pspearman(q, n, false, exact, continuity, upper)
                                                          : pspearman(q, n, true, exact, continuity, upper);
          pv = fmin(2 * ph, 1.0);
        } else {
          pv = pspearman(q, n, alternative == 2, exact, continuity, upper);
        }
      }
    }
  }
  out3[3 * p] = rho;
  out3[3 * p + 1] = pv;
  out3[3 * p + 2] = a.m;
  reasons[p] = reason;
}

}  // namespace

hipError_t launch_cor_prep(const CorPrep& cp, int blocks, hipStream_t s) {
  if (cp.S <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cor_prep, dim3((unsigned)blocks), dim3(CT), 0, s, cp);
  return hipGetLastError();
}

hipError_t launch_cor_tile(const CorPrep& cp, int diag, CorAcc* acc, hipStream_t s) {
  if (cp.S <= 0) return hipSuccess;
  (void)hipGetLastError();
  const int64_t nb = (cp.S + 63) / 64;
  hipLaunchKernelGGL(k_cor_tile, dim3((unsigned)(nb * (nb + 1) / 2)), dim3(CT), 0, s, cp.Z, cp.n, cp.S, diag, cp.cnt,
                     cp.colss, cp.colsum, cp.flags, acc);
  return hipGetLastError();
}

hipError_t launch_cor_dots(const CorPrep& cp, int pairwise, const int32_t* pi, const int32_t* pj, int64_t P, CorAcc* acc,
                           hipStream_t s) {
  if (P <= 0) return hipSuccess;
  (void)hipGetLastError();
  const int64_t blocks = std::min<int64_t>((P + 3) / 4, 65536);
  if (pairwise)
    hipLaunchKernelGGL(k_cor_dots<true>, dim3((unsigned)blocks), dim3(CT), 0, s, cp.X, cp.n, cp.ld, pi, pj, P, cp.cnt,
                       cp.colss, cp.colsum, cp.flags, acc);
  else
    hipLaunchKernelGGL(k_cor_dots<false>, dim3((unsigned)blocks), dim3(CT), 0, s, cp.Z, cp.n, cp.n, pi, pj, P, cp.cnt,
                       cp.colss, cp.colsum, cp.flags, acc);
  return hipGetLastError();
}

hipError_t launch_cor_spearman_pw(const CorPrep& cp, const int32_t* pi, const int32_t* pj, int64_t P, int blocks,
                                  int32_t* scratch, CorAcc* acc, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cor_spearman_pw, dim3((unsigned)blocks), dim3(CT), 0, s, cp, pi, pj, P, scratch, acc);
  return hipGetLastError();
}

hipError_t launch_cor_epilogue(const CorAcc* acc, int64_t P, int method, int pairwise, int alternative, int continuity,
                               const uint32_t* prho_upper, double* out3, int32_t* reasons, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cor_epilogue, dim3((unsigned)((P + CT - 1) / CT)), dim3(CT), 0, s, acc, P, method, pairwise,
                     alternative, continuity, prho_upper, out3, reasons);
  return hipGetLastError();
}

}  // namespace icikt
