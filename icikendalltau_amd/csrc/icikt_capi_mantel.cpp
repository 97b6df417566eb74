// icikt_capi_mantel.cpp -- host side of icikt_mantel_f64 / _in / _csc: the Mantel test (Mantel 1967; vegan::mantel,
// skbio.stats.distance.mantel) of the dissimilarity 1 - raw against another matrix of the same samples, with its
// permutation test, on the device (icikt_mantel.hip).  `other` -- one finite double per pair, in combn order -- crosses
// PCIe once, before the first block: it passes through the key planes, which are free until the first fold, and ends
// as a symmetric S x S table of 32-bit integers (its doubled ranks, or its fixed-point values).  Then the whole combn
// triangle runs through the pair engine in blocks of rows; each block's raw values are kept as sortable keys
// (launch_median_keep).  After the last block the keys become integers as well (ranked as ANOSIM ranks them, or
// quantised), and the permutations -- the identity first, then the caller's -- cross PCIe in batches as rows of
// halfwords and run through the permutation kernel, each batch's kernel behind its copy on the context's stream.
//
// The rule (icikt_mantel.hip and icikt_mantel.h state the device's half; DESIGN.md section 28 the whole): this file
// returns integers only.  T of every labelling as two limbs, the moments sum x, sum x^2, sum y, sum y^2 as limbs, and
// n_ge / n_le: without an NA pair the denominator of r does not depend on the permutation, so T(pi) >= T_obs is
// r(pi) >= r_obs, a comparison of 128-bit integers with no margin.  With an NA pair nothing is summed: every T and
// moment is 0 and n_ge = n_le = 0; the permutations are checked all the same.  r itself is the front end's
// (api.mantel_statistic).
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   24 S (S - 1) / 2                               `kept`, `plane_a` and `plane_b` of the workspace (icikt_ctx::sel):
//                                                  first `other`, its keys' sorted copy and its ranks, then the
//                                                  same for x (method pearson uses two of the three)
//   + 4 S^2                                        the table of y (S = 65 535: 17 GB)
//   + 2 048 ceil(P / tile) + 8 (P / 1 024 + 1)     the sort's counters and a scan's aggregates (method spearman)
//   + 2 S ceil(batch / 16) 16 + 16 batch           a batch of permutations as halfwords, and its sums (by default at most
//                                                  64 MB of indices per batch)
// each with the buffers' growth margin of a ninth.  Host memory: one batch of indices, 16 bytes per permutation and
// O(S); the caller's `other` and perms are read where they lie.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"
#include "icikt_mantel.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct MantelArgs {
  icikt::host::SelectArgs shared;
  const double* other;
  int method;
  const int32_t* perms;
  int64_t n_perm;
  int64_t *n_pairs, *t_lo, *t_hi, *moments, *n_ge, *n_le;
};

static_assert(ICIKT_MANTEL_MAX_PERM == 1000000 && ICIKT_MANTEL_MAX_PERM == ICIKT_ANOSIM_MAX_PERM, "the header's limit is checked here");
static_assert(ICIKT_MANTEL_PEARSON == icikt::mantel::METHOD_PEARSON && ICIKT_MANTEL_SPEARMAN == icikt::mantel::METHOD_SPEARMAN,
              "the header's method codes are icikt_mantel.h's");

constexpr int W_Y = 0, W_X = icikt::MANTEL_MOMENTS, W_NA = 2 * icikt::MANTEL_MOMENTS, W_COUNT = W_NA + 1;   // MantelBufs::words

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int mantel_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const MantelArgs& A) {
  icikt::host::SelectCall call{c, "mantel", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits, a sample index is a halfword");
  if (rc) return rc;
  const int64_t S = n_samp;
  const int64_t P = S > 1 ? S * (S - 1) / 2 : 0;
  const bool spearman = A.method == ICIKT_MANTEL_SPEARMAN;
  if (A.method != ICIKT_MANTEL_PEARSON && !spearman)
    return fail(c, ICIKT_E_INVALID, "mantel: method must be pearson (0) or spearman (1)");
  if (A.n_perm < 0) return fail(c, ICIKT_E_INVALID, "mantel: n_perm must not be negative");
  if (A.n_perm > ICIKT_MANTEL_MAX_PERM) return fail(c, ICIKT_E_INVALID, "mantel: n_perm exceeds ICIKT_MANTEL_MAX_PERM (1000000)");
  if (A.n_perm > 0 && !A.perms) return fail(c, ICIKT_E_INVALID, "mantel: null perms with n_perm > 0");
  if (P > 0 && !A.other) return fail(c, ICIKT_E_INVALID, "mantel: null other");
  if (!A.n_pairs) return fail(c, ICIKT_E_INVALID, "mantel: null output (n_pairs)");
  if (!A.t_lo) return fail(c, ICIKT_E_INVALID, "mantel: null output (t_lo)");
  if (!A.t_hi) return fail(c, ICIKT_E_INVALID, "mantel: null output (t_hi)");
  if (!A.moments) return fail(c, ICIKT_E_INVALID, "mantel: null output (moments)");
  if (!A.n_ge) return fail(c, ICIKT_E_INVALID, "mantel: null output (n_ge)");
  if (!A.n_le) return fail(c, ICIKT_E_INVALID, "mantel: null output (n_le)");
  // `other`: every value finite, and the smallest and the largest of them
  double y_lo = 0.0, y_hi = 0.0;
  for (int64_t p = 0; p < P; ++p) {
    const double y = A.other[p];
    if (!std::isfinite(y)) return fail(c, ICIKT_E_INVALID, "mantel: other[" + std::to_string(p) + "] is not finite");
    if (p == 0 || y < y_lo) y_lo = y;
    if (p == 0 || y > y_hi) y_hi = y;
  }
  const double span = y_hi - y_lo;
  if (!spearman && !std::isfinite(span)) return fail(c, ICIKT_E_INVALID, "mantel: the span of other is not finite");
  const int y_exp = icikt::mantel::span_exponent(span);
  // perms: every row a permutation of 0 .. S - 1.  The gather of the permutation kernel follows these indices: nothing
  // is uploaded before all of them have passed here (stage_labellings tests the range once more on the way)
  std::vector<int32_t> identity;
  try {
    std::vector<int64_t> seen((size_t)S, -1);
    for (int64_t q = 0; q < A.n_perm; ++q) {
      const int32_t* row = A.perms + (size_t)q * (size_t)S;
      for (int64_t s = 0; s < S; ++s) {
        const int32_t v = row[s];
        const bool inside = icikt::host::label_in_range(v, S);
        if (inside && seen[(size_t)v] != q) {
          seen[(size_t)v] = q;
          continue;
        }
        const std::string at = "mantel: perms[" + std::to_string(q) + "][" + std::to_string(s) + "] = " + std::to_string(v);
        return fail(c, ICIKT_E_INVALID, inside ? at + " occurs twice" : at + " is outside 0 .. S - 1 (S = " + std::to_string(S) + ")");
      }
    }
    identity.resize((size_t)S);
    for (int64_t s = 0; s < S; ++s) identity[(size_t)s] = (int32_t)s;
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "mantel: host allocation failed");
  }
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int64_t n_lab = 1 + A.n_perm;     // the identity, then the permutations
  int64_t n_na = 0;
  unsigned long long h_words[W_COUNT] = {};
  std::vector<unsigned long long> tlo, thi;   // per labelling.  The outputs are written once nothing can fail any more
  try {
    tlo.assign((size_t)n_lab, 0ull);
    thi.assign((size_t)n_lab, 0ull);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "mantel: host allocation failed");
  }
  auto write_outputs = [&]() {
    A.n_pairs[0] = P - n_na;
    A.n_pairs[1] = n_na;
    for (int64_t q = 0; q < n_lab; ++q) { A.t_lo[q] = (int64_t)tlo[(size_t)q]; A.t_hi[q] = (int64_t)thi[(size_t)q]; }
    for (int k = 0; k < icikt::MANTEL_MOMENTS; ++k) {   // x's four limbs, then y's
      A.moments[k] = n_na ? 0 : (int64_t)h_words[W_X + k];
      A.moments[icikt::MANTEL_MOMENTS + k] = n_na ? 0 : (int64_t)h_words[W_Y + k];
    }
    int64_t ge = 0, le = 0;
    if (n_na == 0)
      for (int64_t q = 1; q < n_lab; ++q) {
        const int cmp = icikt::mantel::compare_sums(tlo[(size_t)q], thi[(size_t)q], tlo[0], thi[0]);
        ge += cmp >= 0;
        le += cmp <= 0;
      }
    *A.n_ge = ge;
    *A.n_le = le;
  };
  if (n_samp == 0) {   // no column, no pair, no index to check
    write_outputs();
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  PairBlocks blocks = PairBlocks::rows(S, budget);
  const long long tile = icikt::padj_tile(P, c->plan_ov.padjtile > 0 ? c->plan_ov.padjtile : 0);
  const int strip = c->plan_ov.anostrip > 0 ? c->plan_ov.anostrip : icikt::ANO_STRIP_DEFAULT;
  icikt::host::Labellings labs;      // a permutation costs an upload its indices: 2 S bytes
  rc = icikt::host::select_labellings_begin(call, identity.data(), (int)S, A.perms, A.n_perm, 2 * S, &labs);
  if (rc) return rc;
  const size_t sums = (size_t)labs.plan.groups_max * icikt::ANO_PB;   // a batch's sums, in whole groups

  auto& mb = c->mantel;
  auto& ws = c->sel;   // kept, plane_a, plane_b: first y's, then x's
  HIPCHK(c, ws.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.plane_a.reserve((size_t)std::max<int64_t>(P, 1)));
  if (spearman) {
    HIPCHK(c, ws.plane_b.reserve((size_t)std::max<int64_t>(P, 1)));
    HIPCHK(c, ws.total.reserve(1));
    HIPCHK(c, ws.dhist.reserve(8 * 256));
  }
  HIPCHK(c, mb.table.reserve((size_t)S * (size_t)S));
  HIPCHK(c, mb.words.reserve(W_COUNT));
  HIPCHK(c, mb.t_lo.reserve(sums));
  HIPCHK(c, mb.t_hi.reserve(sums));
  const uint32_t flags = A.shared.flags;

  std::vector<unsigned long long> h_lo, h_hi;
  try {
    h_lo.resize(sums);
    h_hi.resize(sums);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "mantel: host allocation failed");
  }

  // the keys in `kept` (x's, or those of -y), all P of them values: their doubled ranks.  *ranks is the plane they are in
  auto rank_kept = [&](const unsigned long long* h_dhist, unsigned long long** ranks) -> int {
    HIPCHK(c, hipMemcpyAsync(ws.plane_a.p, ws.kept.p, (size_t)P * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    unsigned long long* src = nullptr;   // kept stays in pair order for the rank pass: its copy is what is sorted
    const int r = icikt::host::select_sort(c, P, tile, h_dhist, ws.plane_a.p, ws.plane_b.p, &src, ranks);
    if (r) return r;
    HIPCHK(c, icikt::launch_anosim_rank(ws.kept.p, src, P, P, *ranks, c->stream));
    return ICIKT_SUCCESS;
  };
  // the valid keys and the digit table of `kept`, waited for
  auto count_kept = [&](unsigned long long* h_total, unsigned long long* h_dhist) -> int {
    HIPCHK(c, hipMemsetAsync(ws.total.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(ws.dhist.p, 0, 8 * 256 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, icikt::launch_anosim_count(ws.kept.p, P, ws.total.p, ws.dhist.p, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_total, ws.total.p, sizeof *h_total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_dhist, ws.dhist.p, 8 * 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICIKT_SUCCESS;
  };

  icikt::host::SelectSteps steps;
  // y: `other` into the kept plane, its integers into the table; the planes are x's afterwards
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(mb.words.p, 0, W_COUNT * sizeof(unsigned long long), c->stream));
    if (P == 0) return ICIKT_SUCCESS;
    int r = icikt::host::upload_sync(c, ws.kept.p, A.other, (size_t)P * sizeof(double));
    if (r) return r;
    r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    unsigned long long* yv = ws.plane_a.p;
    if (spearman) {
      HIPCHK(c, icikt::launch_mantel_ykeys(ws.kept.p, P, c->stream));
      unsigned long long h_total = 0ull, h_dhist[8 * 256];
      r = count_kept(&h_total, h_dhist);   // (the digit table of y's keys: a wait before the first block)
      if (r) return r;
      if (h_total != (unsigned long long)P) return fail(c, ICIKT_E_STATE, "mantel: a key of other is no value");
      r = rank_kept(h_dhist, &yv);
      if (r) return r;
    } else {
      HIPCHK(c, icikt::launch_mantel_yquant(ws.kept.p, P, y_lo, y_exp, yv, c->stream));
    }
    HIPCHK(c, icikt::launch_mantel_moments(yv, P, mb.words.p + W_Y, c->stream));
    HIPCHK(c, icikt::launch_mantel_expand(yv, (int)S, mb.table.p, c->stream));
    return icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    // the NA pairs say whether anything is left to do: the one wait before the permutations
    unsigned long long* xv = ws.plane_a.p;
    unsigned long long h_na = 0ull, h_dhist[8 * 256];
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (spearman) {
      unsigned long long h_total = 0ull;
      r = count_kept(&h_total, h_dhist);
      if (r) return r;
      if (h_total > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "mantel: more values than pairs");
      h_na = (unsigned long long)P - h_total;
    } else {
      HIPCHK(c, icikt::launch_mantel_xquant(ws.kept.p, P, xv, mb.words.p + W_NA, c->stream));
      HIPCHK(c, hipMemcpyAsync(&h_na, mb.words.p + W_NA, sizeof h_na, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (h_na > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "mantel: more NA pairs than pairs");
    }
    n_na = (int64_t)h_na;
    const bool device = P > 0 && n_na == 0;   // an NA pair: nothing is summed, the permutations are still checked
    if (device) {
      if (spearman) {
        r = rank_kept(h_dhist, &xv);
        if (r) return r;
      }
      HIPCHK(c, icikt::launch_mantel_moments(xv, P, mb.words.p + W_X, c->stream));
    }
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(h_words, mb.words.p, sizeof h_words, hipMemcpyDeviceToHost, c->stream));
    // ---- the permutations (select_labellings): T of every one ----
    icikt::host::LabellingSteps per_batch;
    per_batch.launch = [&](int64_t groups, int64_t) -> int {
      const size_t words = (size_t)groups * icikt::ANO_PB;
      HIPCHK(c, hipMemsetAsync(mb.t_lo.p, 0, words * sizeof(unsigned long long), c->stream));
      HIPCHK(c, hipMemsetAsync(mb.t_hi.p, 0, words * sizeof(unsigned long long), c->stream));
      HIPCHK(c, icikt::launch_mantel_perm(xv, mb.table.p, c->labels.p, (int)S, (int)groups, strip, mb.t_lo.p, mb.t_hi.p,
                                          c->stream));
      return ICIKT_SUCCESS;
    };
    per_batch.collect = [&](int64_t q0, int64_t nb) -> int {
      const size_t words = (size_t)((nb + icikt::ANO_PB - 1) / icikt::ANO_PB) * icikt::ANO_PB;
      HIPCHK(c, hipMemcpyAsync(h_lo.data(), mb.t_lo.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(h_hi.data(), mb.t_hi.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (int64_t l = 0; l < nb; ++l) { tlo[(size_t)(q0 + l)] = h_lo[(size_t)l]; thi[(size_t)(q0 + l)] = h_hi[(size_t)l]; }
      return ICIKT_SUCCESS;
    };
    r = icikt::host::select_labellings(call, labs, device, nullptr, per_batch);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the moments, when no batch ran behind them)
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) write_outputs();
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define MANTEL_ARGS MantelArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                               other, method, perms, n_perm, n_pairs, t_lo, t_hi, moments, n_ge, n_le}

extern "C" {

int icikt_mantel_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const double* other, int method, const int32_t* perms, int64_t n_perm, int64_t* n_pairs,
                     int64_t* t_lo, int64_t* t_hi, int64_t* moments, int64_t* n_ge, int64_t* n_le, double* max_taumax,
                     int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return mantel_src(c, MatrixSrc::dense(&v), n_feat, n_samp, MANTEL_ARGS);
}

int icikt_mantel_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                    const double* other, int method, const int32_t* perms, int64_t n_perm, int64_t* n_pairs,
                    int64_t* t_lo, int64_t* t_hi, int64_t* moments, int64_t* n_ge, int64_t* n_le, double* max_taumax,
                    int64_t* reason_counts) {
  return mantel_src(c, MatrixSrc::dense(X), n_feat, n_samp, MANTEL_ARGS);
}

int icikt_mantel_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const double* other, int method, const int32_t* perms, int64_t n_perm, int64_t* n_pairs,
                     int64_t* t_lo, int64_t* t_hi, int64_t* moments, int64_t* n_ge, int64_t* n_le, double* max_taumax,
                     int64_t* reason_counts) {
  return mantel_src(c, MatrixSrc::csc(X), n_feat, n_samp, MANTEL_ARGS);
}

}  // extern "C"
