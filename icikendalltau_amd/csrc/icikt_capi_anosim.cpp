// icikt_capi_anosim.cpp -- host side of icikt_anosim_f64 / _in / _csc: ANOSIM (Clarke 1993; vegan::anosim) of the
// samples' classes under the dissimilarity 1 - raw, with its permutation test, on the device (icikt_anosim.hip).  The
// whole combn triangle runs through the pair engine in blocks of rows; each block's raw values are kept as sortable
// keys (8 bytes per pair, launch_median_keep) before the next block overwrites them.  After the last block the plane's
// valid keys M and digit table come back in the call's one wait before the labellings; a copy of the plane is sorted
// (launch_padj_sort_pass, the digits all keys share left out), every pair gets its doubled average rank r2, and the
// labellings -- the observed one first, then the caller's permutations -- cross PCIe in batches and run through the
// permutation kernel, each batch's kernel behind its copy on the context's stream.
//
// The rule (icikt_anosim.hip states the device's half): with T2 = M (M + 1), W2 the sum of r2 over the within-class
// values of a labelling, nW their count and nB = M - nW,
//   R = (T2 nW - W2 M) / (nW nB M) = ((M + 1) nW - W2) / (nW nB),
// undefined when nW = 0 or nB = 0.  Two labellings are compared by cross-multiplication: a = (M + 1) nW - W2 is below
// 2^63 in magnitude (W2 <= T2 < 2^63, nW <= M < 2^31) and d = nW nB at most M^2 / 4 < 2^60, so a d' fits a signed
// 128-bit integer with room to spare.  The comparison is exact; no margin is subtracted.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   24 S (S - 1) / 2                               the kept keys in pair order, their sorted copy, and the plane the
//                                                  sort ping-pongs it with, which takes the doubled ranks (S = 65 535:
//                                                  51 GB): `kept`, `plane_a` and `plane_b` of the workspace
//                                                  (icikt_ctx::sel, shared with the other entries)
//   + 2 048 ceil(P / tile)                         the sort's (digit, tile) counters (the workspace's `counts`)
//   + 8 (max(P, 256 tiles) / 1 024 + 1)            a scan's chunk aggregates (its `agg`)
//   + 2 S ceil(batch / 16) 16 + 16 batch           a batch of labellings as halfwords, and its sums (by default at most
//                                                  64 MB of labels per batch)
//   + 4 S + 16 n_class + 16 KB                     the observed labelling, its per-class sums, the digit table
// each with the buffers' growth margin of a ninth.  Host memory: one batch of labels, 16 bytes per labelling and
// O(S + n_class); the caller's perm_cls is read once, where it lies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct AnosimArgs {
  icikt::host::SelectArgs shared;
  const int32_t* cls;
  int n_class;
  const int32_t* perm_cls;
  int64_t n_perm;
  int64_t *n_pairs, *w2, *nw, *n_ge, *n_undefined, *class_w2, *class_nw;
};

static_assert(ICIKT_ANOSIM_MAX_PERM == 1000000 && ICIKT_ANOSIM_MAX_CLASSES == 65535, "the header's limits are checked here");

// R(p) >= R(o) for two labellings with a statistic (nW > 0 and nB > 0 in both), exactly
bool stat_ge(int64_t M, int64_t w2p, int64_t nwp, int64_t w2o, int64_t nwo) {
  const __int128 ap = (__int128)(M + 1) * nwp - w2p, ao = (__int128)(M + 1) * nwo - w2o;
  const __int128 dp = (__int128)nwp * (M - nwp), d_o = (__int128)nwo * (M - nwo);
  return ap * d_o >= ao * dp;
}

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int anosim_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const AnosimArgs& A) {
  icikt::host::SelectCall call{c, "anosim", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits, a label is a halfword");
  if (rc) return rc;
  rc = icikt::host::select_check_labellings(call, A.cls, A.n_class, ICIKT_ANOSIM_MAX_CLASSES, "a label travels as a halfword",
                                            A.perm_cls, A.n_perm);
  if (rc) return rc;
  const int C = A.cls ? A.n_class : 1;   // a null cls: one class, n_class ignored
  if (!A.n_pairs) return fail(c, ICIKT_E_INVALID, "anosim: null output (n_pairs)");
  if (!A.w2) return fail(c, ICIKT_E_INVALID, "anosim: null output (w2)");
  if (!A.nw) return fail(c, ICIKT_E_INVALID, "anosim: null output (nw)");
  if (!A.n_ge) return fail(c, ICIKT_E_INVALID, "anosim: null output (n_ge)");
  if (!A.n_undefined) return fail(c, ICIKT_E_INVALID, "anosim: null output (n_undefined)");
  if (!A.class_w2) return fail(c, ICIKT_E_INVALID, "anosim: null output (class_w2)");
  if (!A.class_nw) return fail(c, ICIKT_E_INVALID, "anosim: null output (class_nw)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int64_t S = n_samp;
  const int64_t P = S > 1 ? S * (S - 1) / 2 : 0;
  const int64_t n_lab = 1 + A.n_perm;     // the observed labelling, then the permutations
  int64_t M = 0;
  std::vector<int64_t> w2, nw, cw2, cnw;  // per labelling; per class.  The outputs are written once nothing can fail any more
  try {
    w2.assign((size_t)n_lab, 0);
    nw.assign((size_t)n_lab, 0);
    cw2.assign((size_t)C, 0);
    cnw.assign((size_t)C, 0);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "anosim: host allocation failed");
  }
  auto write_outputs = [&]() {
    A.n_pairs[0] = M;
    A.n_pairs[1] = P - M;
    for (int64_t q = 0; q < n_lab; ++q) { A.w2[q] = w2[(size_t)q]; A.nw[q] = nw[(size_t)q]; }
    for (int k = 0; k < C; ++k) { A.class_w2[k] = cw2[(size_t)k]; A.class_nw[k] = cnw[(size_t)k]; }
    const bool obs = nw[0] > 0 && nw[0] < M;
    int64_t ge = 0, undef = 0;
    for (int64_t q = 1; q < n_lab; ++q) {
      if (!(nw[(size_t)q] > 0 && nw[(size_t)q] < M)) { ++undef; continue; }
      if (obs && stat_ge(M, w2[(size_t)q], nw[(size_t)q], w2[0], nw[0])) ++ge;
    }
    *A.n_ge = ge;
    *A.n_undefined = undef;
  };
  if (n_samp == 0) {   // no column, no pair, no label to check
    write_outputs();
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  PairBlocks blocks = PairBlocks::rows(S, budget);
  const long long tile = icikt::padj_tile(P, c->plan_ov.padjtile > 0 ? c->plan_ov.padjtile : 0);
  const int strip = c->plan_ov.anostrip > 0 ? c->plan_ov.anostrip : icikt::ANO_STRIP_DEFAULT;
  icikt::host::Labellings labs;      // a labelling costs an upload its labels: 2 S bytes
  rc = icikt::host::select_labellings_begin(call, A.cls, A.n_class, A.perm_cls, A.n_perm, 2 * S, &labs);
  if (rc) return rc;
  const size_t sums = (size_t)labs.plan.groups_max * icikt::ANO_PB;   // a batch's sums, in whole groups

  auto& ab = c->ano;
  auto& ws = c->sel;   // kept, plane_a, plane_b: the keys, their sorted copy, the ranks; the sort's scratch is select_sort's
  HIPCHK(c, ws.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.plane_a.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.plane_b.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.total.reserve(1));
  HIPCHK(c, ws.dhist.reserve(8 * 256));
  HIPCHK(c, ab.class_sums.reserve(2 * (size_t)C));
  HIPCHK(c, ab.cls.reserve((size_t)S));
  HIPCHK(c, ab.w2.reserve(sums));
  HIPCHK(c, ab.nw.reserve(sums));
  const uint32_t flags = A.shared.flags;

  std::vector<unsigned long long> h_w2, h_nw, h_class;
  try {
    h_w2.resize(sums);
    h_nw.resize(sums);
    h_class.resize(2 * (size_t)C);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "anosim: host allocation failed");
  }

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(ws.total.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(ws.dhist.p, 0, 8 * 256 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(ab.class_sums.p, 0, 2 * (size_t)C * sizeof(unsigned long long), c->stream));
    return icikt::host::upload_sync(c, ab.cls.p, labs.obs.data(), (size_t)S * sizeof(int32_t));
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    // M says whether anything is left to do, the digit table which digits to sort by: the one wait before the labellings
    unsigned long long h_total = 0ull, h_dhist[8 * 256];
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_anosim_count(ws.kept.p, P, ws.total.p, ws.dhist.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h_total, ws.total.p, sizeof h_total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_dhist, ws.dhist.p, sizeof h_dhist, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_total > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "anosim: more values than pairs");
    M = (int64_t)h_total;
    const bool device = M > 0;          // without a value every sum is 0: the labels are still checked
    const bool count_nw = M < P;        // an NA pair: nW is counted; else it follows from the class sizes
    unsigned long long* ranks = nullptr;
    if (device) {
      r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
      if (r) return r;
      HIPCHK(c, hipMemcpyAsync(ws.plane_a.p, ws.kept.p, (size_t)P * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
      unsigned long long* src = nullptr;   // kept stays in pair order for the rank pass: its copy is what is sorted
      r = icikt::host::select_sort(c, P, tile, h_dhist, ws.plane_a.p, ws.plane_b.p, &src, &ranks);
      if (r) return r;                  // (the doubled ranks take the plane the sort has left free)
      HIPCHK(c, icikt::launch_anosim_rank(ws.kept.p, src, P, M, ranks, c->stream));
      HIPCHK(c, icikt::launch_anosim_classes(ranks, ab.cls.p, (int)S, ab.class_sums.p, ab.class_sums.p + C, c->stream));
      r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
      if (r) return r;
      HIPCHK(c, hipMemcpyAsync(h_class.data(), ab.class_sums.p, 2 * (size_t)C * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, c->stream));
    }
    // ---- the labellings (select_labellings): W2 of every one, and nW where the class sizes do not give it ----
    icikt::host::LabellingSteps per_batch;
    per_batch.launch = [&](int64_t groups, int64_t) -> int {
      const size_t words = (size_t)groups * icikt::ANO_PB;
      HIPCHK(c, hipMemsetAsync(ab.w2.p, 0, words * sizeof(unsigned long long), c->stream));
      HIPCHK(c, hipMemsetAsync(ab.nw.p, 0, words * sizeof(unsigned long long), c->stream));
      HIPCHK(c, icikt::launch_anosim_perm(ranks, c->labels.p, (int)S, (int)groups, strip, count_nw ? 1 : 0, ab.w2.p, ab.nw.p,
                                          c->stream));
      return ICIKT_SUCCESS;
    };
    per_batch.collect = [&](int64_t q0, int64_t nb) -> int {
      const size_t words = (size_t)((nb + icikt::ANO_PB - 1) / icikt::ANO_PB) * icikt::ANO_PB;
      HIPCHK(c, hipMemcpyAsync(h_w2.data(), ab.w2.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      if (count_nw)
        HIPCHK(c, hipMemcpyAsync(h_nw.data(), ab.nw.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (int64_t l = 0; l < nb; ++l) {
        w2[(size_t)(q0 + l)] = (int64_t)h_w2[(size_t)l];
        if (count_nw) nw[(size_t)(q0 + l)] = (int64_t)h_nw[(size_t)l];
      }
      return ICIKT_SUCCESS;
    };
    r = icikt::host::select_labellings(call, labs, device, device && !count_nw ? nw.data() : nullptr, per_batch);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the per-class sums, when no batch ran behind them)
    if (device)
      for (int k = 0; k < C; ++k) { cw2[(size_t)k] = (int64_t)h_class[(size_t)k]; cnw[(size_t)k] = (int64_t)h_class[(size_t)C + k]; }
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) write_outputs();
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define ANOSIM_ARGS AnosimArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                               cls, n_class, perm_cls, n_perm, n_pairs, w2, nw, n_ge, n_undefined, class_w2, class_nw}

extern "C" {

int icikt_anosim_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm, int64_t* n_pairs,
                     int64_t* w2, int64_t* nw, int64_t* n_ge, int64_t* n_undefined, int64_t* class_w2,
                     int64_t* class_nw, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return anosim_src(c, MatrixSrc::dense(&v), n_feat, n_samp, ANOSIM_ARGS);
}

int icikt_anosim_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                    const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm, int64_t* n_pairs,
                    int64_t* w2, int64_t* nw, int64_t* n_ge, int64_t* n_undefined, int64_t* class_w2, int64_t* class_nw,
                    double* max_taumax, int64_t* reason_counts) {
  return anosim_src(c, MatrixSrc::dense(X), n_feat, n_samp, ANOSIM_ARGS);
}

int icikt_anosim_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm, int64_t* n_pairs,
                     int64_t* w2, int64_t* nw, int64_t* n_ge, int64_t* n_undefined, int64_t* class_w2,
                     int64_t* class_nw, double* max_taumax, int64_t* reason_counts) {
  return anosim_src(c, MatrixSrc::csc(X), n_feat, n_samp, ANOSIM_ARGS);
}

}  // extern "C"
