// icikt_capi_pcoa.cpp -- host side of icikt_pcoa_f64 / _in / _csc: the principal coordinates (classical scaling; Gower
// 1966; vegan::wcmdscale, skbio's pcoa) of the samples under the dissimilarity 1 - raw: the k algebraically largest
// eigenvalues of the Gower-centred table of squared dissimilarities with orthonormal eigenvectors, found on the device
// (icikt_pcoa.hip).  The whole combn triangle runs through the pair engine in blocks of rows; each block's raw values
// are kept as sortable keys (8 bytes per pair, launch_median_keep) before the next block overwrites them.
//
// The rule (icikt_pcoa.hip states the device's half; DESIGN.md section 27 the whole).  After the last block
// k_pcoa_rows sums PERMANOVA's integers q (icikt_fixed.h) per sample; the call's one mid-call wait brings the row sums
// and the NA count to the host, which turns them into the means m_i = R_i / (S 2^50) and m-bar = T / (S^2 2^50), one
// correctly rounded conversion each (icikt_ritz.h).  k_pcoa_centre writes G, and a block Krylov iteration with full
// reorthogonalisation and Rayleigh-Ritz finds the pairs: per step one application of G to the newest block, the
// coefficients against the whole basis (they are the new columns of the projected matrix H = Q^T G Q), the L x L
// eigen-problem on the host (icikt_ritz.h), the residuals |G y - theta y| on the device from the stored image G Q,
// and -- unless every residual is within tol |G|_F or the basis is full -- the new block: G's image orthogonalised
// against the basis twice, then column by column within itself, a column whose norm falls below the breakdown
// threshold dropped.  A step that drops every column has found an invariant subspace.  The work is bounded by
// max_basis; there is no restart.  A pair without a raw (n_na > 0) makes every double NA; the integers are returned.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   8 S (S - 1) / 2       the kept keys in pair order: `kept` of the workspace (icikt_ctx::sel)
//   + 8 S^2               the centred table (S = 65 535: 34 GB)
//   + 16 S max_basis      the basis and its image, + 8 S (64 + 2 k) for a block and the Ritz vectors with their image
// each with the buffers' growth margin of a ninth.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_fixed.h"
#include "icikt_host.h"
#include "icikt_ritz.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct PcoaArgs {
  icikt::host::SelectArgs shared;
  int k;
  double tol;
  int max_basis;
  const double* start;
  int64_t *n_pairs, *q_total, *row_lo, *row_hi;
  double *eigenvalues, *vectors, *residuals, *frobenius, *min_ritz;
  int64_t* solver;
  double* gower;
};

static_assert(ICIKT_PCOA_MAX_K == icikt::PCOA_MAX_BLOCK && ICIKT_PCOA_MAX_BASIS == icikt::PCOA_MAX_BASIS,
              "the header's limits are the kernels'");

double na_real() {
  double v;
  const unsigned long long b = icikt::host::R_NA_BITS;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int pcoa_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const PcoaArgs& A) {
  icikt::host::SelectCall call{c, "pcoa", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits");
  if (rc) return rc;
  if (n_samp < 2) return fail(c, ICIKT_E_INVALID, "pcoa: n_samp must be at least 2");
  const int64_t k_cap = std::min<int64_t>(n_samp - 1, ICIKT_PCOA_MAX_K);
  if (A.k < 1 || A.k > k_cap)
    return fail(c, ICIKT_E_INVALID, "pcoa: k must be in 1 .. min(n_samp - 1, 64)");
  if (!(A.tol > 0.0) || !std::isfinite(A.tol)) return fail(c, ICIKT_E_INVALID, "pcoa: tol must be positive and finite");
  if (A.max_basis != 0 && A.max_basis < A.k)
    return fail(c, ICIKT_E_INVALID, "pcoa: max_basis must be 0 (the default) or at least k");
  if (!A.start) return fail(c, ICIKT_E_INVALID, "pcoa: null start block");
  const struct { const void* p; const char* name; } outs[] = {
      {A.n_pairs, "n_pairs"}, {A.q_total, "q_total"}, {A.row_lo, "row_lo"}, {A.row_hi, "row_hi"},
      {A.eigenvalues, "eigenvalues"}, {A.vectors, "vectors"}, {A.residuals, "residuals"}, {A.frobenius, "frobenius"},
      {A.min_ritz, "min_ritz"}, {A.solver, "solver"}};
  for (const auto& o : outs)
    if (!o.p) return fail(c, ICIKT_E_INVALID, std::string("pcoa: null output (") + o.name + ")");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int S = (int)n_samp, k = A.k;
  const int64_t P = (int64_t)S * (S - 1) / 2;
  int maxb = A.max_basis ? A.max_basis : std::max(8 * k, 128);
  maxb = std::min(std::min(maxb, (int)ICIKT_PCOA_MAX_BASIS), S);
  const double eps = std::ldexp(1.0, -52);
  const size_t SS = (size_t)S * (size_t)S, Sk = (size_t)S * (size_t)k;

  // what the call returns: written to the caller's arrays once nothing can fail any more
  std::vector<unsigned long long> rlo, rhi;
  std::vector<double> mean, H, Hc, w, Z, Zk, theta, res2, coef, lam, resid;
  std::vector<int32_t> flags;
  try {
    rlo.assign((size_t)S, 0ull);
    rhi.assign((size_t)S, 0ull);
    mean.assign((size_t)S + 1, 0.0);
    H.assign((size_t)maxb * maxb, 0.0);
    Hc.assign((size_t)maxb * maxb, 0.0);
    w.assign((size_t)maxb, 0.0);
    Z.assign((size_t)maxb * maxb, 0.0);
    Zk.assign((size_t)maxb * k, 0.0);
    theta.assign((size_t)k, 0.0);
    res2.assign((size_t)std::max(k, S), 0.0);
    coef.assign((size_t)maxb * icikt::PCOA_MAX_BLOCK, 0.0);
    lam.assign((size_t)k, na_real());
    resid.assign((size_t)k, na_real());
    flags.assign(icikt::PCOA_MAX_BLOCK, 0);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "pcoa: host allocation failed");
  }
  unsigned long long h_tot[icikt::PMV_TOTALS] = {0ull, 0ull, 0ull};
  icikt::ritz::u128 T = 0;
  double frob = na_real(), min_ritz = na_real();
  int64_t n_basis = 0, n_apply = 0, converged = 0;
  bool na_result = false;

  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  PairBlocks blocks = PairBlocks::rows(S, budget);
  auto& pb = c->pcoa;
  auto& ws = c->sel;   // kept: the keys
  HIPCHK(c, ws.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, pb.row_lo.reserve((size_t)S));
  HIPCHK(c, pb.row_hi.reserve((size_t)S));
  HIPCHK(c, pb.totals.reserve(icikt::PMV_TOTALS));
  HIPCHK(c, pb.mean.reserve((size_t)S + 1));
  HIPCHK(c, pb.table.reserve(SS));
  HIPCHK(c, pb.basis.reserve((size_t)S * maxb));
  HIPCHK(c, pb.image.reserve((size_t)S * maxb));
  HIPCHK(c, pb.block.reserve((size_t)S * icikt::PCOA_MAX_BLOCK));
  HIPCHK(c, pb.y.reserve(Sk));
  HIPCHK(c, pb.gy.reserve(Sk));
  HIPCHK(c, pb.coef.reserve((size_t)maxb * icikt::PCOA_MAX_BLOCK));
  HIPCHK(c, pb.z.reserve((size_t)maxb * k + (size_t)k));
  HIPCHK(c, pb.small.reserve((size_t)std::max(S, (int)icikt::PCOA_MAX_BLOCK) + 1));
  HIPCHK(c, pb.flags.reserve(icikt::PCOA_MAX_BLOCK));
  const uint32_t flags_arg = A.shared.flags;
  hipStream_t st = nullptr;   // (set in finish: select_run may move the context to the caller's stream state first)

  auto t_begin = [&]() { return icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags_arg); };
  auto t_end = [&]() { return icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags_arg); };
  // the end of a timed group of launches, a small download queued behind it, and the wait
  auto fetch = [&](void* dst, const void* src, size_t bytes) -> int {
    int r = t_end();
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return t_begin();
  };

  // Orthonormalise the n_cols columns of pb.block within themselves, in column order: column j against the columns
  // before it, then against the L columns of the basis once more and against the columns before it again, then its
  // norm; below thr it is zeroed and dropped.  The pass against the basis is not a repetition of the block's two: they
  // left the block orthogonal to the basis to eps times the norm a column HAD, and the pass against its neighbours can
  // take twelve orders off that norm -- normalised as it stood, such a column would lean into the basis by eps times
  // the ratio (a rank-1 table shows it: its Ritz values then leave the spectrum).  The kept columns go to the basis
  // from column L on, at most `room` of them.  *n_kept: how many.
  auto orth_block = [&](int n_cols, double thr, int L, int room, int* n_kept) -> int {
    double* B = pb.block.p;
    for (int j = 0; j < n_cols; ++j) {
      double* col = B + (size_t)j * S;
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && L > 0) {   // what the first pass left of the column may be far smaller than the column was
          HIPCHK(c, icikt::launch_pcoa_qtw(pb.basis.p, L, col, S, 1, L, pb.coef.p, st));
          HIPCHK(c, icikt::launch_pcoa_axz(pb.basis.p, L, pb.coef.p, L, S, 1, 1, col, st));
        }
        if (j > 0) {
          HIPCHK(c, icikt::launch_pcoa_qtw(B, j, col, S, 1, j, pb.coef.p, st));
          HIPCHK(c, icikt::launch_pcoa_axz(B, j, pb.coef.p, j, S, 1, 1, col, st));
        }
      }
      HIPCHK(c, icikt::launch_pcoa_sumsq(col, S, S, 1, pb.small.p, st));
      HIPCHK(c, icikt::launch_pcoa_scale(col, S, pb.small.p, thr * thr, pb.flags.p + j, st));
    }
    int r = fetch(flags.data(), pb.flags.p, (size_t)n_cols * sizeof(int32_t));
    if (r) return r;
    int kept = 0;
    for (int j = 0; j < n_cols && kept < room; ++j)
      if (flags[(size_t)j]) {
        HIPCHK(c, hipMemcpyAsync(pb.basis.p + (size_t)(L + kept) * S, B + (size_t)j * S, (size_t)S * sizeof(double),
                                 hipMemcpyDeviceToDevice, st));
        ++kept;
      }
    *n_kept = kept;
    return ICIKT_SUCCESS;
  };

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(pb.totals.p, 0, icikt::PMV_TOTALS * sizeof(unsigned long long), c->stream));
    return ICIKT_SUCCESS;
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    st = c->stream;
    int r = t_begin();
    if (r) return r;
    HIPCHK(c, icikt::launch_pcoa_rows(ws.kept.p, S, pb.row_lo.p, pb.row_hi.p, pb.totals.p, st));
    r = t_end();
    if (r) return r;
    // the one wait for the integers
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_tot, pb.totals.p, sizeof h_tot, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rlo.data(), pb.row_lo.p, (size_t)S * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rhi.data(), pb.row_hi.p, (size_t)S * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (h_tot[icikt::PMV_T_NA] > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "pcoa: more NA pairs than pairs");
    T = 0;
    for (int i = 0; i < S; ++i) T += ((icikt::ritz::u128)rhi[(size_t)i] << 32) + rlo[(size_t)i];
    if (T & 1) return fail(c, ICIKT_E_STATE, "pcoa: the row sums do not add up to twice a total");
    if (h_tot[icikt::PMV_T_NA] > 0) {   // every pair is needed: the doubles are NA, the integers are returned
      na_result = true;
      return ICIKT_SUCCESS;
    }
    // the means
    const icikt::ritz::u128 scale = (icikt::ritz::u128)1 << icikt::fixed::FRAC_BITS;
    for (int i = 0; i < S; ++i)
      mean[(size_t)i] = icikt::ritz::ratio_to_double(((icikt::ritz::u128)rhi[(size_t)i] << 32) + rlo[(size_t)i],
                                                     (icikt::ritz::u128)S * scale);
    mean[(size_t)S] = icikt::ritz::ratio_to_double(T, (icikt::ritz::u128)S * (icikt::ritz::u128)S * scale);
    r = icikt::host::upload_sync(c, pb.mean.p, mean.data(), ((size_t)S + 1) * sizeof(double));
    if (!r) r = icikt::host::upload_sync(c, pb.block.p, A.start, Sk * sizeof(double));
    if (!r) r = t_begin();
    if (r) return r;
    double* const G = pb.table.p;
    double* const Q = pb.basis.p;
    double* const GQ = pb.image.p;
    HIPCHK(c, icikt::launch_pcoa_centre(ws.kept.p, pb.mean.p, pb.mean.p + S, S, G, st));
    // |G|_F once, in a fixed order: every row's sum of squares, then their sum; and the start block's column norms
    HIPCHK(c, icikt::launch_pcoa_sumsq(G, S, S, S, pb.small.p, st));
    HIPCHK(c, icikt::launch_pcoa_sum(pb.small.p, S, pb.small.p + S, st));
    r = fetch(&frob, pb.small.p + S, sizeof(double));
    if (r) return r;
    frob = std::sqrt(frob);
    if (!std::isfinite(frob)) return fail(c, ICIKT_E_STATE, "pcoa: the centred table is not finite");
    HIPCHK(c, icikt::launch_pcoa_sumsq(pb.block.p, S, S, k, pb.small.p, st));
    r = fetch(res2.data(), pb.small.p, (size_t)k * sizeof(double));
    if (r) return r;
    double start_max = 0.0;
    for (int j = 0; j < k; ++j) {
      if (!std::isfinite(res2[(size_t)j])) return fail(c, ICIKT_E_INVALID, "pcoa: the start block is not finite");
      start_max = std::max(start_max, std::sqrt(res2[(size_t)j]));
    }
    // the breakdown thresholds: 4 S eps times the largest norm a column can have had, and for an
    // image under G not below S 2^-48, what the roundings of G's own cells can add up to over a unit vector
    const double thr_start = 4.0 * S * eps * start_max;
    const double thr = std::max(4.0 * S * eps * frob, std::ldexp((double)S, -48));
    int L = 0, La = 0, kept = 0;
    r = orth_block(k, thr_start, 0, maxb, &kept);
    if (r) return r;
    if (kept < k) return fail(c, ICIKT_E_INVALID, "pcoa: the start block has fewer than k independent columns");
    L = kept;
    bool done = false;
    while (!done) {
      const int nb = L - La;   // the newest block: not applied yet
      HIPCHK(c, icikt::launch_pcoa_apply(G, Q + (size_t)La * S, S, nb, GQ + (size_t)La * S, st));
      n_apply += 1;
      HIPCHK(c, icikt::launch_pcoa_qtw(Q, L, GQ + (size_t)La * S, S, nb, L, pb.coef.p, st));
      r = fetch(coef.data(), pb.coef.p, (size_t)L * nb * sizeof(double));
      if (r) return r;
      // H [maxb][maxb]: column La + j of Q^T G Q is coef[. + L j]; inside the block the two estimates of a cell are averaged
      for (int j = 0; j < nb; ++j)
        for (int l = 0; l < L; ++l) {
          const int cj = La + j;
          double v = coef[(size_t)l + (size_t)L * j];
          if (l >= La) v = 0.5 * (v + coef[(size_t)cj + (size_t)L * (l - La)]);
          H[(size_t)l * maxb + cj] = v;
          H[(size_t)cj * maxb + l] = v;
        }
      La = L;
      // Rayleigh-Ritz over the L columns
      for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) Hc[(size_t)i * L + j] = H[(size_t)i * maxb + j];
      if (!icikt::ritz::sym_eig(Hc.data(), L, w.data(), Z.data()))
        return fail(c, ICIKT_E_STATE, "pcoa: the projected eigen-problem did not converge");
      for (int a = 0; a < k; ++a) {          // the k largest, descending: sym_eig's are ascending
        theta[(size_t)a] = w[(size_t)(L - 1 - a)];
        for (int l = 0; l < L; ++l) Zk[(size_t)l + (size_t)L * a] = Z[(size_t)l * L + (L - 1 - a)];
      }
      min_ritz = w[0];
      r = t_end();
      if (!r) r = icikt::host::upload_sync(c, pb.z.p, Zk.data(), (size_t)L * k * sizeof(double));
      if (!r) r = icikt::host::upload_sync(c, pb.z.p + (size_t)maxb * k, theta.data(), (size_t)k * sizeof(double));
      if (!r) r = t_begin();
      if (r) return r;
      HIPCHK(c, icikt::launch_pcoa_axz(Q, L, pb.z.p, L, S, k, 0, pb.y.p, st));
      HIPCHK(c, icikt::launch_pcoa_axz(GQ, L, pb.z.p, L, S, k, 0, pb.gy.p, st));
      HIPCHK(c, icikt::launch_pcoa_resid(pb.gy.p, pb.y.p, pb.z.p + (size_t)maxb * k, S, k, pb.small.p, st));
      r = fetch(res2.data(), pb.small.p, (size_t)k * sizeof(double));
      if (r) return r;
      bool all_in = true;
      for (int a = 0; a < k; ++a) {
        resid[(size_t)a] = std::sqrt(res2[(size_t)a]);
        all_in = all_in && resid[(size_t)a] <= A.tol * frob;
      }
      n_basis = L;
      if (all_in) { converged = 1; break; }
      if (L >= maxb) break;                  // the basis is full: the best pairs, not converged
      // the next block: G's image of the newest one, against the basis twice, then within itself
      HIPCHK(c, hipMemcpyAsync(pb.block.p, GQ + (size_t)(L - nb) * S, (size_t)S * nb * sizeof(double),
                               hipMemcpyDeviceToDevice, st));
      for (int pass = 0; pass < 2; ++pass) {
        HIPCHK(c, icikt::launch_pcoa_qtw(Q, L, pb.block.p, S, nb, L, pb.coef.p, st));
        HIPCHK(c, icikt::launch_pcoa_axz(Q, L, pb.coef.p, L, S, nb, 1, pb.block.p, st));
      }
      r = orth_block(nb, thr, L, maxb - L, &kept);
      if (r) return r;
      if (kept == 0) { converged = 1; done = true; }   // every column dropped: an invariant subspace
      L += kept;
    }
    for (int a = 0; a < k; ++a) lam[(size_t)a] = theta[(size_t)a];
    HIPCHK(c, icikt::launch_pcoa_sign(pb.y.p, S, k, st));
    r = t_end();
    if (r) return r;
    // the large results go to the caller's arrays behind everything that can refuse the call
    r = icikt::host::download(c, A.vectors, pb.y.p, Sk * sizeof(double));
    if (!r && A.gower) r = icikt::host::download(c, A.gower, G, SS * sizeof(double));
    return r;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (rc) return rc;
  const unsigned long long n_na = h_tot[icikt::PMV_T_NA];
  const icikt::ritz::u128 Qt = T >> 1;
  A.n_pairs[0] = P - (int64_t)n_na;
  A.n_pairs[1] = (int64_t)n_na;
  A.q_total[0] = (int64_t)(unsigned long long)(Qt & 0xFFFFFFFFull);
  A.q_total[1] = (int64_t)(unsigned long long)(Qt >> 32);
  for (int i = 0; i < S; ++i) { A.row_lo[i] = (int64_t)rlo[(size_t)i]; A.row_hi[i] = (int64_t)rhi[(size_t)i]; }
  for (int a = 0; a < k; ++a) { A.eigenvalues[a] = lam[(size_t)a]; A.residuals[a] = resid[(size_t)a]; }
  *A.frobenius = frob;
  *A.min_ritz = min_ritz;
  A.solver[0] = n_basis;
  A.solver[1] = n_apply;
  A.solver[2] = converged;
  if (na_result) {
    const double na = na_real();
    std::fill(A.vectors, A.vectors + Sk, na);
    if (A.gower) std::fill(A.gower, A.gower + SS, na);
  }
  return ICIKT_SUCCESS;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define PCOA_ARGS PcoaArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                           k, tol, max_basis, start, n_pairs, q_total, row_lo, row_hi, eigenvalues, vectors, residuals,    \
                           frobenius, min_ritz, solver, gower}

extern "C" {

int icikt_pcoa_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                   int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int k, double tol,
                   int max_basis, const double* start, int64_t* n_pairs, int64_t* q_total, int64_t* row_lo,
                   int64_t* row_hi, double* eigenvalues, double* vectors, double* residuals, double* frobenius,
                   double* min_ritz, int64_t* solver, double* gower, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return pcoa_src(c, MatrixSrc::dense(&v), n_feat, n_samp, PCOA_ARGS);
}

int icikt_pcoa_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                  int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int k, double tol,
                  int max_basis, const double* start, int64_t* n_pairs, int64_t* q_total, int64_t* row_lo,
                  int64_t* row_hi, double* eigenvalues, double* vectors, double* residuals, double* frobenius,
                  double* min_ritz, int64_t* solver, double* gower, double* max_taumax, int64_t* reason_counts) {
  return pcoa_src(c, MatrixSrc::dense(X), n_feat, n_samp, PCOA_ARGS);
}

int icikt_pcoa_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int k, double tol,
                   int max_basis, const double* start, int64_t* n_pairs, int64_t* q_total, int64_t* row_lo,
                   int64_t* row_hi, double* eigenvalues, double* vectors, double* residuals, double* frobenius,
                   double* min_ritz, int64_t* solver, double* gower, double* max_taumax, int64_t* reason_counts) {
  return pcoa_src(c, MatrixSrc::csc(X), n_feat, n_samp, PCOA_ARGS);
}

int icikt_pcoa_apply_dev(icikt_ctx* c, const double* d_G, const double* d_V, int64_t n_samp, int b, double* d_W) {
  if (!c) return ICIKT_E_INVALID;
  if (n_samp < 1 || n_samp > ICIKT_TOPK_MAX_SAMPLES) return fail(c, ICIKT_E_INVALID, "pcoa_apply: n_samp must be in 1 .. 65535");
  if (b < 1 || b > ICIKT_PCOA_MAX_K) return fail(c, ICIKT_E_INVALID, "pcoa_apply: b must be in 1 .. 64");
  if (!d_G || !d_V || !d_W) return fail(c, ICIKT_E_INVALID, "pcoa_apply: null device array");
  const int rc = icikt::host::use_device(c);
  if (rc) return rc;
  HIPCHK(c, icikt::launch_pcoa_apply(d_G, d_V, (int)n_samp, b, d_W, c->stream));
  return ICIKT_SUCCESS;
}

}  // extern "C"
