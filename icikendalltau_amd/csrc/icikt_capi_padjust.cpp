// icikt_capi_padjust.cpp -- host side of icikt_padjust_f64 / _in / _csc: R's p.adjust (bonferroni, holm, hochberg, BH)
// over the p-values of all C(S, 2) pairs, on the device (icikt_padjust.hip).  The combn triangle runs through the pair
// engine in blocks of whole rows; each block's p-values are kept as sortable keys (8 bytes per pair).  After the last
// block the number of tests m and the keys' digit table come back in the call's one wait before its end; the host
// leaves out the digits all keys share, the device sorts the plane, adjusts the first m positions, finds the cut-offs
// of the alphas and compacts the table of distinct p-values -- the table's extent stays on the device.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   16 S (S - 1) / 2                               the kept keys and the plane the sort ping-pongs them with, which
//                                                  takes the adjusted values (S = 65 535: 34 GB): `kept` and `plane_a`
//                                                  of the workspace (icikt_ctx::sel, shared with the other entries)
//   + 2 048 ceil(P / tile)                         the sort's (digit, tile) counters: 2 MB per 1 024 tiles, at most
//                                                  65 536 tiles (the workspace's `counts`)
//   + 8 (max(P, 256 tiles) / 1 024 + 1)            a scan's chunk aggregates (its `agg`)
//   + 16 min(max_table, P)                         the table
//   + 16 KB                                        the digit table (the workspace's `dhist`), the alphas, the cut-offs' record
// each with the buffers' growth margin of a ninth.  Host memory: O(1), never O(pairs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct PadjArgs {
  icikt::host::SelectArgs shared;
  int method;
  const double* alpha;
  int n_alpha;
  int64_t max_table;
  int64_t *n_tests, *n_rejected;
  double *p_cutoff, *table;
  int64_t* n_table;
};

static_assert(ICIKT_ADJUST_BONFERRONI == icikt::PADJ_BONFERRONI && ICIKT_ADJUST_HOLM == icikt::PADJ_HOLM &&
                  ICIKT_ADJUST_HOCHBERG == icikt::PADJ_HOCHBERG && ICIKT_ADJUST_BH == icikt::PADJ_BH &&
                  ICIKT_ADJUST_MAX_ALPHA == icikt::PADJ_MAX_ALPHA,
              "the header's constants are the device's");

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int padjust_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const PadjArgs& A) {
  icikt::host::SelectCall call{c, "padjust", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the number of tests and a test's position stay below 2^31");
  if (rc) return rc;
  if (A.method != ICIKT_ADJUST_BONFERRONI && A.method != ICIKT_ADJUST_HOLM && A.method != ICIKT_ADJUST_HOCHBERG &&
      A.method != ICIKT_ADJUST_BH)
    return fail(c, ICIKT_E_INVALID, "padjust: method " + std::to_string(A.method) +
                                        " is none of ICIKT_ADJUST_BONFERRONI, _HOLM, _HOCHBERG, _BH (0 .. 3)");
  if (A.n_alpha < 1 || A.n_alpha > ICIKT_ADJUST_MAX_ALPHA)
    return fail(c, ICIKT_E_INVALID, "padjust: n_alpha must be in 1 .. ICIKT_ADJUST_MAX_ALPHA (16)");
  if (!A.alpha) return fail(c, ICIKT_E_INVALID, "padjust: null alpha");
  for (int a = 0; a < A.n_alpha; ++a)
    if (!(A.alpha[a] >= 0.0 && A.alpha[a] <= 1.0))
      return fail(c, ICIKT_E_INVALID, "padjust: alpha[" + std::to_string(a) + "] = " + std::to_string(A.alpha[a]) +
                                          " is outside [0, 1]");
  if (A.max_table < 0) return fail(c, ICIKT_E_INVALID, "padjust: max_table must not be negative");
  if (!A.n_tests) return fail(c, ICIKT_E_INVALID, "padjust: null output (n_tests)");
  if (!A.n_rejected) return fail(c, ICIKT_E_INVALID, "padjust: null output (n_rejected)");
  if (!A.p_cutoff) return fail(c, ICIKT_E_INVALID, "padjust: null output (p_cutoff)");
  if (!A.n_table) return fail(c, ICIKT_E_INVALID, "padjust: null output (n_table)");
  if (A.max_table > 0 && !A.table) return fail(c, ICIKT_E_INVALID, "padjust: null output (table)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int64_t S = n_samp;
  const int64_t P = S * (S - 1) / 2;
  int64_t m = 0, n_table = 0;
  unsigned long long h_cut[icikt::PADJ_CUT_WORDS] = {};
  // every output from what was found; without a test every count is 0 and every cut-off NA
  auto write_outputs = [&]() {
    A.n_tests[0] = m;
    A.n_tests[1] = P - m;
    for (int a = 0; a < A.n_alpha; ++a) {
      A.n_rejected[a] = m > 0 ? (int64_t)h_cut[a] : 0;
      const unsigned long long bits = m > 0 ? h_cut[icikt::PADJ_MAX_ALPHA + a] : icikt::host::R_NA_BITS;
      std::memcpy(&A.p_cutoff[a], &bits, sizeof(double));
    }
    *A.n_table = n_table;
  };
  if (n_samp == 0) {   // no column, no pair
    write_outputs();
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  PairBlocks blocks = PairBlocks::rows(S, budget);
  const long long tile = icikt::padj_tile(P, c->plan_ov.padjtile > 0 ? c->plan_ov.padjtile : 0);
  const int64_t cap = std::min<int64_t>(A.max_table, P);   // (there are no more distinct p-values than pairs)
  auto& pb = c->padj;
  auto& ws = c->sel;   // kept and plane_a: the keys and the sort; the sort's counters and aggregates are select_sort's
  HIPCHK(c, ws.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.plane_a.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.total.reserve(1));
  HIPCHK(c, ws.dhist.reserve(8 * 256));
  HIPCHK(c, pb.cut.reserve(icikt::PADJ_CUT_WORDS));
  HIPCHK(c, pb.n_table.reserve(1));
  HIPCHK(c, pb.alpha.reserve(icikt::PADJ_MAX_ALPHA));
  HIPCHK(c, pb.table.reserve((size_t)std::max<int64_t>(2 * cap, 1)));
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    const int r = icikt::host::upload_sync(c, pb.alpha.p, A.alpha, (size_t)A.n_alpha * sizeof(double));
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(ws.total.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(ws.dhist.p, 0, 8 * 256 * sizeof(unsigned long long), c->stream));
    return ICIKT_SUCCESS;
  };
  // a block's p-values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int {
    HIPCHK(c, icikt::launch_padj_fold(c->d_out4.p, c->d_reasons.p, b.count, b.begin, (int)S, ws.kept.p, ws.total.p,
                                      ws.dhist.p, c->stream));
    return ICIKT_SUCCESS;
  };
  steps.finish = [&](unsigned long long* red) -> int {
    // m sizes the scans, the digit table says which digits to sort by: the one wait inside the call
    unsigned long long h_total = 0ull, h_dhist[8 * 256];
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h_total, ws.total.p, sizeof h_total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_dhist, ws.dhist.p, sizeof h_dhist, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (P == 0 || h_total == 0ull) return ICIKT_SUCCESS;
    if (h_total > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "padjust: more tests than pairs");
    m = (int64_t)h_total;
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    unsigned long long *src = nullptr, *dst = nullptr;
    r = icikt::host::select_sort(c, P, tile, h_dhist, ws.kept.p, ws.plane_a.p, &src, &dst);
    if (r) return r;
    double* const adj = reinterpret_cast<double*>(dst);   // the adjusted values take the plane the sort has left free
    HIPCHK(c, icikt::launch_padj_adjust(src, m, A.method, adj, reinterpret_cast<double*>(ws.agg.p), c->stream));
    HIPCHK(c, icikt::launch_padj_cut(adj, src, m, pb.alpha.p, A.n_alpha, pb.cut.p, c->stream));
    HIPCHK(c, icikt::launch_padj_table(src, adj, m, pb.cut.p + 2 * icikt::PADJ_MAX_ALPHA, cap, pb.table.p, ws.agg.p,
                                       pb.n_table.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    unsigned long long h_n_table = 0ull;
    HIPCHK(c, hipMemcpyAsync(h_cut, pb.cut.p, sizeof h_cut, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h_n_table, pb.n_table.p, sizeof h_n_table, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    n_table = (int64_t)h_n_table;
    const int64_t n_out = std::min<int64_t>(n_table, cap);   // the slots behind them are left as they are
    if (n_out > 0) {
      HIPCHK(c, hipMemcpyAsync(A.table, pb.table.p, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(A.table + A.max_table, pb.table.p + cap, (size_t)n_out * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) write_outputs();
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define PADJ_ARGS PadjArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                           method, alpha, n_alpha, max_table, n_tests, n_rejected, p_cutoff, table, n_table}

extern "C" {

int icikt_padjust_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                      int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int method,
                      const double* alpha, int n_alpha, int64_t max_table, int64_t* n_tests, int64_t* n_rejected,
                      double* p_cutoff, double* table, int64_t* n_table, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return padjust_src(c, MatrixSrc::dense(&v), n_feat, n_samp, PADJ_ARGS);
}

int icikt_padjust_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int method,
                     const double* alpha, int n_alpha, int64_t max_table, int64_t* n_tests, int64_t* n_rejected,
                     double* p_cutoff, double* table, int64_t* n_table, double* max_taumax, int64_t* reason_counts) {
  return padjust_src(c, MatrixSrc::dense(X), n_feat, n_samp, PADJ_ARGS);
}

int icikt_padjust_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                      int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int method,
                      const double* alpha, int n_alpha, int64_t max_table, int64_t* n_tests, int64_t* n_rejected,
                      double* p_cutoff, double* table, int64_t* n_table, double* max_taumax, int64_t* reason_counts) {
  return padjust_src(c, MatrixSrc::csc(X), n_feat, n_samp, PADJ_ARGS);
}

}  // extern "C"
