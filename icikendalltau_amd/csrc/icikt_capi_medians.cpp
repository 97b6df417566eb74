// icikt_capi_medians.cpp -- host side of icikt_class_medians_f64 / _in / _csc: every sample's median ICI-Kendall-tau
// over the other samples of its class, reduced on the device (icikt_medians.hip).  Only the within-class pairs run
// through the pair engine, in blocks; each block's raw values are kept as sortable keys (8 bytes per pair) before the
// next block overwrites them, and the select kernel reads the kept plane once the last block is through.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), 8 P bytes of kept keys
// in the workspace's `kept` plane (icikt_ctx::sel, shared with the other entries) for the P = sum over the classes of
// m (m - 1) / 2 computed pairs (one class of 65 535 samples: 17 GB) and 36 S bytes:
// the index arrays (position in class, class size, the class's first pair as int64: 16) and the results (20), each
// with the buffers' growth margin of a ninth.  Host memory: O(S) for the classes and O(block) for a slice's pi / pj, never O(P).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct MedianArgs {
  icikt::host::SelectArgs shared;
  const int32_t* cls;
  int n_class, scale_max;
  double* med2;
  int32_t* n_valid;
};

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int medians_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const MedianArgs& A) {
  icikt::host::SelectCall call{c, "class_medians", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "a class's pairs are indexed from 32-bit positions");
  if (rc) return rc;
  rc = icikt::host::select_check_classes(call, A.cls, A.n_class);
  if (rc) return rc;
  if (n_samp > 0 && !A.med2) return fail(c, ICIKT_E_INVALID, "class_medians: null output (med2)");
  rc = icikt::host::select_check_args(call);
  if (rc || n_samp == 0) return rc;
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const int64_t S = n_samp;
  icikt::host::ClassIndex ci;
  try { ci = icikt::host::class_index(A.cls, S); } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "class_medians: host allocation failed");
  }
  // one class (all samples in it: the combn triangle): blocks of whole rows; several: slices of the explicit list
  PairBlocks blocks = ci.runs.run.size() == 1 ? PairBlocks::rows(S, budget) : PairBlocks::slices(&ci.runs, ci.total, budget);
  const int stage = c->plan_ov.medlds >= 0 ? c->plan_ov.medlds : icikt::MEDIAN_STAGE_MAX;
  auto& md = c->med;
  HIPCHK(c, c->sel.kept.reserve((size_t)std::max<int64_t>(ci.total, 1)));
  HIPCHK(c, md.pos.reserve((size_t)S));
  HIPCHK(c, md.size.reserve((size_t)S));
  HIPCHK(c, md.base.reserve((size_t)S));
  HIPCHK(c, md.med2.reserve(2 * (size_t)S));
  HIPCHK(c, md.n_valid.reserve((size_t)S));
  const icikt::MedianClasses mc{md.pos.p, md.size.p, md.base.p};
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    int r = icikt::host::upload_sync(c, md.pos.p, ci.pos.data(), (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, md.size.p, ci.size.data(), (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, md.base.p, ci.base.data(), (size_t)S * sizeof(long long));
    return r;
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_median_select(mc, c->sel.kept.p, c->d_red.p, (int)S, A.scale_max ? 1 : 0, stage, md.med2.p,
                                          md.n_valid.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, A.med2, md.med2.p, 2 * (size_t)S * sizeof(double));
    if (!r && A.n_valid) r = icikt::host::download(c, A.n_valid, md.n_valid.p, (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::select_download_red(c, red);
    return r;
  };
  return icikt::host::select_run(call, blocks, steps);
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define MEDIAN_ARGS MedianArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                               cls, n_class, scale_max, med2, n_valid}

extern "C" {

int icikt_class_medians_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                            const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                            int alternative, int continuity, uint32_t flags, int scale_max, double* med2,
                            int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return medians_src(c, MatrixSrc::dense(&v), n_feat, n_samp, MEDIAN_ARGS);
}

int icikt_class_medians_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                           int n_global_na, const int32_t* cls, int n_class, int perspective, int alternative,
                           int continuity, uint32_t flags, int scale_max, double* med2, int32_t* n_valid,
                           double* max_taumax, int64_t* reason_counts) {
  return medians_src(c, MatrixSrc::dense(X), n_feat, n_samp, MEDIAN_ARGS);
}

int icikt_class_medians_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp,
                            const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                            int alternative, int continuity, uint32_t flags, int scale_max, double* med2,
                            int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return medians_src(c, MatrixSrc::csc(X), n_feat, n_samp, MEDIAN_ARGS);
}

}  // extern "C"
