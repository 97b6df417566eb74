// icikt_capi_classmat.cpp -- host side of icikt_class_matrix_f64 / _in / _csc: every sample's median ICI-Kendall-tau
// to every class, reduced on the device (icikt_classmat.hip).  The whole combn triangle runs through the pair engine
// in blocks of rows; each block's raw values are kept as sortable keys (8 bytes per pair, launch_median_keep) before
// the next block overwrites them, and the select kernel reads the kept plane once the last block is through.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), 8 S (S - 1) / 2 bytes
// of kept keys in the workspace's `kept` plane (icikt_ctx::sel, shared with the other entries; 65 535 samples: 17 GB),
// 4 (S + n_class + 1) bytes of member list and class ranges and 20 S n_class bytes of results, each with the buffers'
// growth margin of a ninth.  Host memory: O(S + n_class), never O(S^2).
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

struct ClassMatArgs {
  icikt::host::SelectArgs shared;
  const int32_t* cls;
  int n_class, scale_max;
  double* med2;
  int32_t* n_valid;
};

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int classmat_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const ClassMatArgs& A) {
  icikt::host::SelectCall call{c, "class_matrix", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits");
  if (rc) return rc;
  rc = icikt::host::select_check_classes(call, A.cls, A.n_class, icikt::CLASS_MATRIX_MAX_CLASSES,
                                         "the classes are the second dimension of the select kernel's grid");
  if (rc) return rc;
  if (n_samp > 0 && !A.med2) return fail(c, ICIKT_E_INVALID, "class_matrix: null output (med2)");
  rc = icikt::host::select_check_args(call);
  if (rc || n_samp == 0) return rc;
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const int64_t S = n_samp;
  const int C = A.cls ? A.n_class : 1;   // a null cls: one class, n_class ignored
  const size_t SC = (size_t)S * (size_t)C;
  // the samples sorted stably by class (class_index) and each class's range in that list; an empty class: first[c] == first[c + 1]
  icikt::host::ClassIndex ci;
  std::vector<int32_t> first;
  try {
    ci = icikt::host::class_index(A.cls, S);
    first.assign((size_t)C + 1, 0);
    if (A.cls) for (int64_t s = 0; s < S; ++s) ++first[(size_t)A.cls[s] + 1];
    else first[1] = (int32_t)S;
    for (int k = 0; k < C; ++k) first[(size_t)k + 1] += first[(size_t)k];
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "class_matrix: host allocation failed");
  }
  const std::vector<int32_t>& member = ci.runs.member;
  PairBlocks blocks = PairBlocks::rows(S, budget);
  const int stage = c->plan_ov.medlds >= 0 ? c->plan_ov.medlds : icikt::MEDIAN_STAGE_MAX;
  auto& cm = c->cmat;
  HIPCHK(c, c->sel.kept.reserve((size_t)std::max<int64_t>(blocks.total, 1)));
  HIPCHK(c, cm.member.reserve((size_t)S));
  HIPCHK(c, cm.first.reserve((size_t)C + 1));
  HIPCHK(c, cm.med2.reserve(2 * SC));
  HIPCHK(c, cm.n_valid.reserve(SC));
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    int r = icikt::host::upload_sync(c, cm.member.p, member.data(), (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, cm.first.p, first.data(), ((size_t)C + 1) * sizeof(int32_t));
    return r;
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_class_select(cm.member.p, cm.first.p, c->sel.kept.p, c->d_red.p, (int)S, C, A.scale_max ? 1 : 0,
                                         stage, cm.med2.p, cm.n_valid.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, A.med2, cm.med2.p, 2 * SC * sizeof(double));
    if (!r && A.n_valid) r = icikt::host::download(c, A.n_valid, cm.n_valid.p, SC * sizeof(int32_t));
    if (!r) r = icikt::host::select_download_red(c, red);
    return r;
  };
  return icikt::host::select_run(call, blocks, steps);
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define CLASSMAT_ARGS ClassMatArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                                   cls, n_class, scale_max, med2, n_valid}

extern "C" {

int icikt_class_matrix_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                           const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                           int alternative, int continuity, uint32_t flags, int scale_max, double* med2,
                           int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return classmat_src(c, MatrixSrc::dense(&v), n_feat, n_samp, CLASSMAT_ARGS);
}

int icikt_class_matrix_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                          int n_global_na, const int32_t* cls, int n_class, int perspective, int alternative,
                          int continuity, uint32_t flags, int scale_max, double* med2, int32_t* n_valid,
                          double* max_taumax, int64_t* reason_counts) {
  return classmat_src(c, MatrixSrc::dense(X), n_feat, n_samp, CLASSMAT_ARGS);
}

int icikt_class_matrix_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp,
                           const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                           int alternative, int continuity, uint32_t flags, int scale_max, double* med2,
                           int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return classmat_src(c, MatrixSrc::csc(X), n_feat, n_samp, CLASSMAT_ARGS);
}

}  // extern "C"
