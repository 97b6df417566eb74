// icikt_epilogue.hip -- what runs on the pair kernels' counts (gfx950): nothing here is on the hot path.
//
//   k2_epilogue      one pair per lane: tau, tau_max, completeness, variance, z, p (kendallc.cpp:280-335), with
//                    perspective = "local" DERIVED from the global counts; R's pnorm on the device
//   k_missingness    pairwise_completeness: popcount of mask OR, one pair per wave
//   k_mask_pairs     kt_fast(use = "pairwise.complete.obs"): a pair's two columns with the incomplete rows dropped
//   k_out_stats, k_assemble, k_assemble_diag, k_fill_combn   the full-matrix assembly (scale_and_reshape)
// and their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "icikt_device.h"
#include "icikt_wave.h"

namespace icikt {

// ------------------------------------------------------------------------------------------------
// K2: epilogue, one pair per lane
// ------------------------------------------------------------------------------------------------
// R's pnorm (libR nmath pnorm_both): W. J. Cody, Math. Comp. 23 (1969) 631-637.
__device__ void pnorm_both_dev(double x, double& cum, double& ccum) {
  const double a[5] = {2.2352520354606839287, 161.02823106855587881, 1067.6894854603709582,
                       18154.981253343561249, 0.065682337918207449113};
  const double b[4] = {47.20258190468824187, 976.09855173777669322, 10260.932208618978205,
                       45507.789335026729956};
  const double c[9] = {0.39894151208813466764, 8.8831497943883759412, 93.506656132177855979,
                       597.27027639480026226,  2494.5375852903726711, 6848.1904505362823326,
                       11602.651437647350124,  9842.7148383839780218, 1.0765576773720192317e-8};
  const double d[8] = {22.266688044328115691, 235.38790178262499861, 1519.377599407554805,
                       6485.558298266760755,  18615.571640885098091, 34900.952721145977266,
                       38912.003286093271411, 19685.429676859990727};
  const double pp[6] = {0.21589853405795699,    0.1274011611602473639, 0.022235277870649807,
                        0.001421619193227893466, 2.9112874951168792e-5, 0.02307344176494017303};
  const double qq[5] = {1.28426009614491121,   0.468238212480865118, 0.0659881378689285515,
                        0.00378239633202758244, 7.29751555083966205e-5};
  if (x != x) { cum = x; ccum = x; return; }
  const double y = fabs(x);
  double xnum, xden, temp, xsq, del;
  if (y <= 0.67448975) {
    if (y > 1.1102230246251565e-16) {
      xsq = x * x;
      xnum = a[4] * xsq;
      xden = xsq;
      for (int i = 0; i < 3; ++i) { xnum = (xnum + a[i]) * xsq; xden = (xden + b[i]) * xsq; }
    } else {
      xnum = xden = 0.0;
    }
    temp = x * (xnum + a[3]) / (xden + b[3]);
    cum = 0.5 + temp;
    ccum = 0.5 - temp;
  } else if (y <= 5.656854249492380195206754896838) {
    xnum = c[8] * y;
    xden = y;
    for (int i = 0; i < 7; ++i) { xnum = (xnum + c[i]) * y; xden = (xden + d[i]) * y; }
    temp = (xnum + c[7]) / (xden + d[7]);
    xsq = trunc(y * 16) / 16;
    del = (y - xsq) * (y + xsq);
    cum = exp(-xsq * xsq * 0.5) * exp(-del * 0.5) * temp;
    ccum = 1.0 - cum;
    if (x > 0.) { temp = cum; cum = ccum; ccum = temp; }
  } else if ((-37.5193 < x && x < 8.2924) || (-8.2924 < x && x < 37.5193)) {
    xsq = 1.0 / (x * x);
    xnum = pp[5] * xsq;
    xden = xsq;
    for (int i = 0; i < 4; ++i) { xnum = (xnum + pp[i]) * xsq; xden = (xden + qq[i]) * xsq; }
    temp = xsq * (xnum + pp[4]) / (xden + qq[4]);
    temp = (0.398942280401432677939946059934 - temp) / y;
    xsq = trunc(x * 16) / 16;
    del = (x - xsq) * (x + xsq);
    cum = exp(-xsq * xsq * 0.5) * exp(-del * 0.5) * temp;
    ccum = 1.0 - cum;
    if (x > 0.) { temp = cum; cum = ccum; ccum = temp; }
  } else {
    if (x > 0) { cum = 1.; ccum = 0.; } else { cum = 0.; ccum = 1.; }
  }
}

__device__ __forceinline__ void pnorm_tails(double z, double& lower, double& upper) {
  if (isinf(z)) { lower = z > 0 ? 1.0 : 0.0; upper = 1.0 - lower; return; }
  pnorm_both_dev(z, lower, upper);
}

// element of count_rank_tie's three sums for one tie group of size t, int32 arithmetic as uint32
__device__ __forceinline__ void tie_terms32(int t, uint32_t& a0, uint32_t& a1, uint32_t& a2) {
  if (t < 2) { a0 = a1 = a2 = 0; return; }
  const uint32_t ut = (uint32_t)t, tt1 = ut * (ut - 1u);
  a0 = tt1; a1 = tt1 * (ut - 2u); a2 = tt1 * (2u * ut + 5u);
}
__device__ __forceinline__ void tie_terms64(long long t, long long& a0, long long& a1, long long& a2) {
  if (t < 2) { a0 = a1 = a2 = 0; return; }
  a0 = t * (t - 1); a1 = t * (t - 1) * (t - 2); a2 = t * (t - 1) * (2 * t + 5);
}

__global__ void __launch_bounds__(256)
k2_epilogue(PrepView pv, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
            const PairRaw* __restrict__ raw, int64_t n_pairs, int perspective, int alternative,
            int continuity, int exact64, double* __restrict__ out4, int64_t* __restrict__ counts,
            int32_t* __restrict__ reasons) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const double NA = __longlong_as_double(0x7FF00000000007A2ll);  // R's NA_real_
  const ColStats sx = *pv.col_stats(pi[p]);
  const ColStats sy = *pv.col_stats(pj[p]);
  const PairRaw rw = (pv.n > 0) ? raw[p] : PairRaw{0ull, 0ull, 0u, 0u};
  const long long n = pv.n;
  const long long cb = rw.c_both;
  const bool local = (perspective == ICIKT_PERSPECTIVE_LOCAL_);

  int reason = 0;
  double o_tau = NA, o_p = NA, o_tmax = NA, o_comp = NA;
  long long cnt[ICIKT_CNT_FIELDS_] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  // kendallc.cpp:190-199; dropping the both-missing rows cannot change "all missing"
  if (sx.nna == n || sy.nna == n) {
    reason = 1;
  } else {
    const long long ne = local ? (n - cb) : n;                               // :180-185, :221
    const long long missing = (long long)sx.nna + sy.nna - (local ? 2 * cb : cb);  // :208-211
    const double completeness = 1.0 - (double)missing / (double)ne;
    // a fill group vanishes under "local" when every member was a both-missing row
    const int kx = sx.ngroups - ((local && sx.nna > 0 && sx.tfill == cb) ? 1 : 0);
    const int ky = sy.ngroups - ((local && sy.nna > 0 && sy.tfill == cb) ? 1 : 0);
    if (ne < 2) {
      reason = 2;                                                            // :224-231
    } else if (kx == 1 || ky == 1) {
      reason = 3;                                                            // :234-244
    } else {
      const long long shrink = local ? cb : 0;
      double xtie, x0, x1, ytie, y0, y1, ntie;
      const long long g = rw.g, g2 = g - shrink;
      const long long others = (long long)rw.ntie - g * (g - 1) / 2;          // joint ties outside the fill/fill cell
      if (exact64) {
        long long a0, a1, a2, b0, b1, b2;
        tie_terms64(sx.tfill, a0, a1, a2); tie_terms64(sx.tfill - shrink, b0, b1, b2);
        xtie = (double)((sx.e0 - a0 + b0) / 2); x0 = (double)((sx.e1 - a1 + b1) / 2); x1 = (double)(sx.e2 - a2 + b2);
        tie_terms64(sy.tfill, a0, a1, a2); tie_terms64(sy.tfill - shrink, b0, b1, b2);
        ytie = (double)((sy.e0 - a0 + b0) / 2); y0 = (double)((sy.e1 - a1 + b1) / 2); y1 = (double)(sy.e2 - a2 + b2);
        ntie = (double)(others + (g2 >= 2 ? g2 * (g2 - 1) / 2 : 0));
      } else {
        uint32_t a0, a1, a2, b0, b1, b2;
        tie_terms32(sx.tfill, a0, a1, a2); tie_terms32((int)(sx.tfill - shrink), b0, b1, b2);
        xtie = (double)((int32_t)(sx.s0 - a0 + b0) / 2); x0 = (double)((int32_t)(sx.s1 - a1 + b1) / 2);
        x1 = (double)(int32_t)(sx.s2 - a2 + b2);
        tie_terms32(sy.tfill, a0, a1, a2); tie_terms32((int)(sy.tfill - shrink), b0, b1, b2);
        ytie = (double)((int32_t)(sy.s0 - a0 + b0) / 2); y0 = (double)((int32_t)(sy.s1 - a1 + b1) / 2);
        y1 = (double)(int32_t)(sy.s2 - a2 + b2);
        // sum((cnt * (cnt - 1)) / 2) in int32 (:267): only a cell of >= 46342 rows can wrap, and a pair has at
        // most one (n <= 65535).  It is the cell of the two columns' largest tie groups: the (fill, fill) cell is
        // known (g); any other one is counted here, row by row -- both columns must have a group that large, rare
        const int32_t cell = (g2 >= 2) ? ((int32_t)((uint32_t)g2 * (uint32_t)(g2 - 1)) / 2) : 0;
        long long rest = others;
        int32_t cell2 = 0;
        const int mgx = (int)((uint32_t)sx.maxgroup >> 16), mgy = (int)((uint32_t)sy.maxgroup >> 16);
        const uint32_t lbx = (uint32_t)sx.maxgroup & 0xFFFFu, lby = (uint32_t)sy.maxgroup & 0xFFFFu;
        const bool fill_fill = (sx.nna > 0 && lbx == 0u) && (sy.nna > 0 && lby == 0u);
        if (mgx >= 46342 && mgy >= 46342 && !fill_fill) {
          const int cx = pi[p], cy = pj[p];
          const uint32_t* rx = pv.rec + ((int64_t)(cx >> 1) * pv.rec_rows) * 2 + (cx & 1);
          const uint32_t* ry = pv.rec + ((int64_t)(cy >> 1) * pv.rec_rows) * 2 + (cy & 1);
          long long c = 0;
          for (int r = 0; r < pv.n; ++r) c += ((rx[2 * r] >> 16) == lbx && (ry[2 * r] >> 16) == lby) ? 1 : 0;
          if (c >= 46342) {
            rest -= c * (c - 1) / 2;
            cell2 = (int32_t)((uint32_t)c * (uint32_t)(c - 1)) / 2;
          }
        }
        ntie = (double)(int32_t)((uint32_t)rest + (uint32_t)cell + (uint32_t)cell2);
      }
      const long long dis = (long long)rw.dis;  // both-missing rows are never discordant
      const long long tot = ne * (ne - 1) / 2;                                // :280
      cnt[0] = ne; cnt[1] = missing; cnt[2] = dis; cnt[3] = (long long)ntie;
      cnt[4] = (long long)xtie; cnt[5] = (long long)ytie; cnt[6] = (long long)x0; cnt[7] = (long long)x1;
      cnt[8] = (long long)y0; cnt[9] = (long long)y1; cnt[10] = tot;
      if (xtie == (double)tot || ytie == (double)tot) {
        reason = 4;                                                           // :291-298
      } else {
        const double dtot = (double)tot;
        const double con_minus_dis = dtot - xtie - ytie + ntie - 2.0 * (double)dis;  // :300
        const double den = sqrt((dtot - xtie) * (dtot - ytie));
        double tau = con_minus_dis / den;
        const double con_plus_dis = dtot - xtie - ytie + ntie;
        const double tau_max = con_plus_dis / den;                            // not clipped (:303)
        if (tau > 1) tau = 1; else if (tau < -1) tau = -1;
        const long long m = ne * (ne - 1);                                    // :310
        const double var = (((double)(m * (2 * ne + 5)) - x1 - y1) / 18 + (2 * xtie * ytie) / (double)m +
                            x0 * y0 / (double)(9 * m * (ne - 2)));            // :311-312
        double s_adj = tau * sqrt(((double)(m / 2) - xtie) * ((double)(m / 2) - ytie));  // :315
        if (continuity) {
          const double sg = s_adj > 0 ? 1.0 : (s_adj == 0 ? 0.0 : -1.0);
          s_adj = sg * (fabs(s_adj) - 1);                                     // :316-319
        }
        const double z = s_adj / sqrt(var);
        double pval = 0.0, plo, pup;
        pnorm_tails(z, plo, pup);
        if (alternative == 1) pval = plo;                                     // "less"
        else if (alternative == 2) pval = pup;                                // "greater"
        else if (alternative == 0) {                                          // "two.sided": 2 * min
          double mn = plo;
          if (!(plo != plo)) { if (pup != pup) mn = pup; else if (pup < mn) mn = pup; }
          pval = 2 * mn;
        }
        o_tau = tau; o_p = pval; o_tmax = tau_max; o_comp = completeness;
      }
    }
  }
  out4[4 * p + 0] = o_tau;
  out4[4 * p + 1] = o_p;
  out4[4 * p + 2] = o_tmax;
  out4[4 * p + 3] = o_comp;
  if (reasons) reasons[p] = reason;
  if (counts) {
    for (int f = 0; f < ICIKT_CNT_FIELDS_; ++f) counts[p * ICIKT_CNT_FIELDS_ + f] = cnt[f];
  }
}

// ------------------------------------------------------------------------------------------------
// pairwise missingness (pairwise_completeness, R/kendalltau.R:611-629): popcount of mask OR
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_missingness(PrepView pv, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, int64_t n_pairs,
              int64_t* __restrict__ missing) {
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // one pair per wave
  if (p >= n_pairs) return;
  const uint32_t lane = lane_id();
  const unsigned long long* ma = pv.col_mask(pi[p]);
  const unsigned long long* mb = pv.col_mask(pj[p]);
  uint32_t c = 0;
  for (int w = lane; w < pv.W; w += 64) c += (uint32_t)__popcll(ma[w] | mb[w]);
  const unsigned long long tot = wave_sum_u64(c);
  if (lane == 0) missing[p] = (int64_t)tot;
}

// ------------------------------------------------------------------------------------------------
// kt_fast(use = "pairwise.complete.obs") (R/kendalltau.R:310-354, 448-545): per pair, rows with a missing value in
// EITHER vector are dropped.  Writes the pair's two columns with both entries of such rows missing; "local" then
// removes exactly those rows (src/kendallc.cpp:180-185) and nothing missing remains.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_mask_pairs(const double* __restrict__ X, int64_t ld, int n, const int32_t* __restrict__ pi,
             const int32_t* __restrict__ pj, int64_t first, int64_t npairs, double* __restrict__ Xp) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const double na = __longlong_as_double(0x7FF8000000000000ll);
  for (int64_t p = blockIdx.y; p < npairs; p += gridDim.y) {   // pair of the chunk (the y-grid is capped: launch_mask_pairs)
    const double a = X[(int64_t)pi[first + p] * ld + i], b = X[(int64_t)pj[first + p] * ld + i];
    const bool drop = (a != a) || (b != b);
    Xp[(2 * p) * (int64_t)n + i] = drop ? na : a;
    Xp[(2 * p + 1) * (int64_t)n + i] = drop ? na : b;
  }
}

// ------------------------------------------------------------------------------------------------
// Full-matrix assembly: scale_and_reshape (R/kendalltau.R:357-421) on the device
// ------------------------------------------------------------------------------------------------
// The reference row-binds the chunks' data.frames, divides raw by max(taumax, na.rm = TRUE) (:368-373), appends one
// row per sample for the diagonal (raw = cor = n_good / max(n_good), pvalue 0, taumax 1, completeness =
// n_good / n_feature, :375-386) and fills five S x S matrices symmetrically by name pair (:390-415): on the host that
// is a 523 776-row data.frame and ten indexed assignments at c4.  Here: one reduction kernel, one scatter kernel,
// one D2H of 5 S^2 doubles.
__device__ __forceinline__ unsigned long long dbl_sortable(double v) {   // monotone in v; 0 is below every double
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dbl_unsortable(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
__device__ __forceinline__ long long col_n_good(const PrepView& pv, const int64_t* n_good, int c) {
  return n_good ? (long long)n_good[c] : (long long)pv.n - pv.col_stats(c)->nexcl;
}

// red[0] = max over the pairs of the sortable key of taumax (NaN skipped; 0 = no pair had one), red[1 + r] = pairs
// with reason code r (0..4), red[6] = max(n_good)
__global__ void __launch_bounds__(256)
k_out_stats(PrepView pv, const double* __restrict__ out4, const int32_t* __restrict__ reasons, int64_t n_pairs,
            const int64_t* __restrict__ n_good, unsigned long long* __restrict__ red) {
  __shared__ unsigned long long sh[8];
  if (threadIdx.x < 8) sh[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long mx = 0ull, mg = 0ull;
  uint32_t rc[5] = {0u, 0u, 0u, 0u, 0u};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += stride) {
    const double t = out4[4 * p + 2];
    if (t == t) mx = max(mx, dbl_sortable(t));
    const int r = reasons ? reasons[p] : 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) rc[k] += (r == k) ? 1u : 0u;
  }
  for (int64_t cc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; cc < pv.n_samp; cc += stride)
    mg = max(mg, (unsigned long long)max(0ll, col_n_good(pv, n_good, (int)cc)));
  atomicMax(&sh[0], mx);
  atomicMax(&sh[6], mg);
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (rc[k]) atomicAdd(&sh[1 + k], (unsigned long long)rc[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMax(&red[0], sh[0]);
    atomicMax(&red[6], sh[6]);
  }
  if (threadIdx.x >= 1 && threadIdx.x <= 5 && sh[threadIdx.x]) atomicAdd(&red[threadIdx.x], sh[threadIdx.x]);
}

// pair p of combn(S, 2): row i holds the pairs (i, i+1 .. S-1) and starts at offset i (2S - i - 1) / 2
__device__ __forceinline__ void combn_pair(int64_t S, int64_t t, int64_t& i, int64_t& j) {
  const double b = 2.0 * (double)S - 1.0;
  i = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  i = max((int64_t)0, min(i, S - 2));
  while (i > 0 && i * (2 * S - i - 1) / 2 > t) --i;
  while ((i + 1) * (2 * S - i - 2) / 2 <= t) ++i;
  j = i + 1 + (t - i * (2 * S - i - 1) / 2);
}
// out5: five S x S matrices, zero-filled by the caller; a thread per pair writes both triangles, then a thread per
// sample the diagonal (the diagonal rows come AFTER the pairs in the reference: they win over a self pair of the list)
__global__ void __launch_bounds__(256)
k_assemble(PrepView pv, const double* __restrict__ out4, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj,
           int64_t n_pairs, const int64_t* __restrict__ n_good, const unsigned long long* __restrict__ red, int scale_max,
           int diag_good, double* __restrict__ out5) {
  const int64_t S = pv.n_samp, SS = S * S;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_pairs) {
    int64_t i, j;
    if (pi) {
      i = pi[t]; j = pj[t];
    } else {
      combn_pair(S, t, i, j);
    }
    const double raw = out4[4 * t + 0], pval = out4[4 * t + 1], tmax = out4[4 * t + 2], comp = out4[4 * t + 3];
    // max(numeric(0), na.rm = TRUE) is -Inf in R
    const double max_cor = red[0] ? dbl_unsortable(red[0]) : -__longlong_as_double(0x7FF0000000000000ll);
    const double cor = scale_max ? raw / max_cor : raw;
    const int64_t a = i + j * S, b2 = j + i * S;
    out5[a] = cor;            out5[b2] = cor;
    out5[SS + a] = raw;       out5[SS + b2] = raw;
    out5[2 * SS + a] = pval;  out5[2 * SS + b2] = pval;
    out5[3 * SS + a] = tmax;  out5[3 * SS + b2] = tmax;
    out5[4 * SS + a] = comp;  out5[4 * SS + b2] = comp;
  }
}
__global__ void __launch_bounds__(256)
k_assemble_diag(PrepView pv, const int64_t* __restrict__ n_good, const unsigned long long* __restrict__ red,
                double* __restrict__ out5) {
  const int64_t S = pv.n_samp, SS = S * S;
  const int64_t cc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cc >= S) return;
  const double g = (double)col_n_good(pv, n_good, (int)cc);
  const double d = g / (double)red[6];                       // n_good / max(n_good)  (0 / 0 = NaN, as in R)
  const int64_t a = cc + cc * S;
  out5[a] = d;
  out5[SS + a] = d;
  out5[2 * SS + a] = 0.0;
  out5[3 * SS + a] = 1.0;
  out5[4 * SS + a] = g / (double)pv.n;                       // frac_complete = n_good / nrow
}

__global__ void __launch_bounds__(256)
k_fill_combn(int32_t* __restrict__ pi, int32_t* __restrict__ pj, int64_t S, int64_t begin, int64_t count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  int64_t i, j;
  combn_pair(S, begin + t, i, j);
  pi[t] = (int32_t)i;
  pj[t] = (int32_t)j;
}
hipError_t launch_fill_combn(int32_t* pi, int32_t* pj, int64_t S, int64_t begin, int64_t count, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_fill_combn, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, pi, pj, S, begin, count);
  return hipGetLastError();
}

hipError_t launch_out_stats(const PrepView& pv, const double* out4, const int32_t* reasons, int64_t n_pairs,
                            const int64_t* n_good, unsigned long long* red, hipStream_t s) {
  (void)hipGetLastError();
  hipError_t e = hipMemsetAsync(red, 0, 8 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  const int64_t work = std::max<int64_t>(n_pairs, pv.n_samp);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (work + 255) / 256));
  hipLaunchKernelGGL(k_out_stats, dim3(blocks), dim3(256), 0, s, pv, out4, reasons, n_pairs, n_good, red);
  return hipGetLastError();
}

hipError_t launch_out_stats_accum(const PrepView& pv, const double* out4, const int32_t* reasons, int64_t n_pairs,
                                  unsigned long long* red, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  (void)hipGetLastError();
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n_pairs + 255) / 256));
  hipLaunchKernelGGL(k_out_stats, dim3(blocks), dim3(256), 0, s, pv, out4, reasons, n_pairs, nullptr, red);
  return hipGetLastError();
}

hipError_t launch_assemble(const PrepView& pv, const double* out4, const int32_t* pi, const int32_t* pj, int64_t n_pairs,
                           const int64_t* n_good, const unsigned long long* red, int scale_max, int diag_good,
                           double* out5, hipStream_t s) {
  const size_t S = (size_t)pv.n_samp;
  if (S == 0) return hipSuccess;
  (void)hipGetLastError();
  hipError_t e = hipMemsetAsync(out5, 0, 5 * S * S * sizeof(double), s);
  if (e != hipSuccess) return e;
  if (n_pairs > 0)
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, pv, out4, pi, pj, n_pairs,
                       n_good, red, scale_max, diag_good, out5);
  if (diag_good)
    hipLaunchKernelGGL(k_assemble_diag, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, pv, n_good, red, out5);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// launchers of the kernels above (called from icikt_capi.cpp)
// ------------------------------------------------------------------------------------------------
// (every launcher first drops whatever error an earlier, unrelated HIP call of the calling thread left behind: the
//  hipGetLastError() after the launch must report THIS launch)
hipError_t launch_k2(const PrepView& pv, const int32_t* pi, const int32_t* pj, const PairRaw* raw,
                     int64_t n_pairs, int perspective, int alternative, int continuity, int exact64,
                     double* out4, int64_t* counts, int32_t* reasons, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  (void)hipGetLastError();
  const int threads = 256;
  const int64_t blocks = (n_pairs + threads - 1) / threads;
  hipLaunchKernelGGL(k2_epilogue, dim3((unsigned)blocks), dim3(threads), 0, s, pv, pi, pj, raw, n_pairs,
                     perspective, alternative, continuity, exact64, out4, counts, reasons);
  return hipGetLastError();
}

hipError_t launch_missingness(const PrepView& pv, const int32_t* pi, const int32_t* pj, int64_t n_pairs,
                              int64_t* missing, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  (void)hipGetLastError();
  const int threads = 256;
  const int64_t blocks = (n_pairs * 64 + threads - 1) / threads;
  hipLaunchKernelGGL(k_missingness, dim3((unsigned)blocks), dim3(threads), 0, s, pv, pi, pj, n_pairs, missing);
  return hipGetLastError();
}

hipError_t launch_mask_pairs(const double* dX, int64_t ld, int n, const int32_t* pi, const int32_t* pj, int64_t first,
                             int64_t npairs, double* dXp, hipStream_t s) {
  if (npairs <= 0 || n <= 0) return hipSuccess;
  (void)hipGetLastError();
  // a chunk holds up to (3 << 29) / (16 n) pairs, millions on short columns: past the y-grid's 65 535 blocks the kernel strides
  hipLaunchKernelGGL(k_mask_pairs, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(npairs, 65535)), dim3(256), 0, s,
                     dX, ld, n, pi, pj, first, npairs, dXp);
  return hipGetLastError();
}

}  // namespace icikt
