// icikt_capi_permdisp.cpp -- host side of icikt_permdisp_f64 / _in / _csc: PERMDISP (Anderson 2006; vegan::betadisper
// with permutest) of the samples' classes under the dissimilarity 1 - raw: every sample's sum of squared dissimilarities
// to every class, on the device (icikt_permdisp.hip).  The whole combn triangle runs through the pair engine in blocks
// of rows; each block's raw values are kept as sortable keys (8 bytes per pair, launch_median_keep) before the next
// block overwrites them.  After the last block one kernel sweeps the kept plane into the S x n_class table, quantising
// on the fly (icikt_fixed.h), and counts the NA pairs and Q; table and totals come back in the call's one wait.
//
// The rule (icikt_permdisp.hip states the device's half; DESIGN.md section 26 the whole).  This file returns integers
// only, and returns them as summed whether or not a pair is NA: the centroid distances are square roots of 84-bit
// integers over squared class sizes, and the statistic is a ratio of sums of those, so the distances, F and the
// permutation test are the front end's (api.permdisp_distance, api.permdisp_statistic), in integers and fractions.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   8 S (S - 1) / 2          the kept keys in pair order (S = 65 535: 17 GB): `kept` of the workspace (icikt_ctx::sel)
//   + 16 S n_class + 4 S     the two limbs of the table and the labels
// each with the buffers' growth margin of a ninth.  Host memory: 16 bytes per cell of S n_class until the call has
// succeeded, which is why that product is capped (ICIKT_PERMDISP_MAX_CELLS: 1 GiB of table).
#include <hip/hip_runtime.h>

#include <algorithm>
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

struct PermdispArgs {
  icikt::host::SelectArgs shared;
  const int32_t* cls;
  int n_class;
  int64_t *n_pairs, *q_total, *t_lo, *t_hi;
};

static_assert(ICIKT_PERMDISP_MAX_CELLS == icikt::DISP_MAX_CELLS && ICIKT_PERMDISP_MAX_CELLS == 67108864,
              "the header's limit is checked here, and the message below spells it out");

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int permdisp_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const PermdispArgs& A) {
  icikt::host::SelectCall call{c, "permdisp", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits");
  if (rc) return rc;
  rc = icikt::host::select_check_classes(call, A.cls, A.n_class, ICIKT_ANOSIM_MAX_CLASSES, "the labels are ANOSIM's and PERMANOVA's");
  if (rc) return rc;
  const int C = A.cls ? A.n_class : 1;   // a null cls: one class, n_class ignored
  if (n_samp * (int64_t)C > ICIKT_PERMDISP_MAX_CELLS)
    return fail(c, ICIKT_E_INVALID, "permdisp: n_samp n_class exceeds ICIKT_PERMDISP_MAX_CELLS (67108864)");
  if (!A.n_pairs) return fail(c, ICIKT_E_INVALID, "permdisp: null output (n_pairs)");
  if (!A.q_total) return fail(c, ICIKT_E_INVALID, "permdisp: null output (q_total)");
  if (!A.t_lo) return fail(c, ICIKT_E_INVALID, "permdisp: null output (t_lo)");
  if (!A.t_hi) return fail(c, ICIKT_E_INVALID, "permdisp: null output (t_hi)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int64_t S = n_samp;
  const int64_t P = S > 1 ? S * (S - 1) / 2 : 0;
  const size_t SC = (size_t)S * (size_t)C;
  unsigned long long h_tot[icikt::PMV_TOTALS] = {0ull, 0ull, 0ull};
  std::vector<unsigned long long> tlo, thi;   // [S][C].  The outputs are written once nothing can fail any more
  std::vector<int32_t> zeros;                 // a null cls
  try {
    tlo.assign(SC, 0ull);
    thi.assign(SC, 0ull);
    if (!A.cls) zeros.assign((size_t)S, 0);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "permdisp: host allocation failed");
  }
  auto write_outputs = [&]() {
    A.n_pairs[0] = P - (int64_t)h_tot[icikt::PMV_T_NA];
    A.n_pairs[1] = (int64_t)h_tot[icikt::PMV_T_NA];
    A.q_total[0] = (int64_t)h_tot[icikt::PMV_T_LO];
    A.q_total[1] = (int64_t)h_tot[icikt::PMV_T_HI];
    for (size_t k = 0; k < SC; ++k) { A.t_lo[k] = (int64_t)tlo[k]; A.t_hi[k] = (int64_t)thi[k]; }
  };
  if (n_samp == 0) {   // no column, no pair, no cell
    write_outputs();
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  PairBlocks blocks = PairBlocks::rows(S, budget);
  const int32_t* h_cls = A.cls ? A.cls : zeros.data();
  auto& db = c->disp;
  auto& ws = c->sel;   // kept: the keys
  HIPCHK(c, ws.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, db.cls.reserve((size_t)S));
  HIPCHK(c, db.t_lo.reserve(SC));
  HIPCHK(c, db.t_hi.reserve(SC));
  HIPCHK(c, db.totals.reserve(icikt::PMV_TOTALS));
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(db.totals.p, 0, icikt::PMV_TOTALS * sizeof(unsigned long long), c->stream));
    return icikt::host::upload_sync(c, db.cls.p, h_cls, (size_t)S * sizeof(int32_t));
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_disp_table(ws.kept.p, db.cls.p, (int)S, C, db.t_lo.p, db.t_hi.p, db.totals.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_tot, db.totals.p, sizeof h_tot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(tlo.data(), db.t_lo.p, SC * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(thi.data(), db.t_hi.p, SC * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_tot[icikt::PMV_T_NA] > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "permdisp: more NA pairs than pairs");
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) write_outputs();
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define PERMDISP_ARGS PermdispArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                                   cls, n_class, n_pairs, q_total, t_lo, t_hi}

extern "C" {

int icikt_permdisp_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                       int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                       const int32_t* cls, int n_class, int64_t* n_pairs, int64_t* q_total, int64_t* t_lo, int64_t* t_hi,
                       double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return permdisp_src(c, MatrixSrc::dense(&v), n_feat, n_samp, PERMDISP_ARGS);
}

int icikt_permdisp_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                      int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                      const int32_t* cls, int n_class, int64_t* n_pairs, int64_t* q_total, int64_t* t_lo, int64_t* t_hi,
                      double* max_taumax, int64_t* reason_counts) {
  return permdisp_src(c, MatrixSrc::dense(X), n_feat, n_samp, PERMDISP_ARGS);
}

int icikt_permdisp_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                       int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                       const int32_t* cls, int n_class, int64_t* n_pairs, int64_t* q_total, int64_t* t_lo, int64_t* t_hi,
                       double* max_taumax, int64_t* reason_counts) {
  return permdisp_src(c, MatrixSrc::csc(X), n_feat, n_samp, PERMDISP_ARGS);
}

}  // extern "C"
