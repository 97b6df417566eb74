// icikt_capi_cross.cpp -- host side of icikt_cross_f64 / _in: the ICI-Kendall-tau of every column of a query matrix
// with every column of a reference matrix, as five Sq x Sr matrices and / or as every query's k best reference columns
// (icikt_cross.hip).  The device matrix holds the query columns, one all-missing padding column when Sq is odd (the
// reference must start on an even column: the pre-pass's tables are interleaved in blocks of two), then the reference
// columns; the rectangle runs through the selection entries' driver (select_run) in blocks of whole query rows
// (PairBlocks::rect), and each block is folded before the next one overwrites its records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct CrossArgs {
  icikt::host::SelectArgs shared;
  int k, scale_max;
  double* out5;
  int32_t* idx;
  double* out5k;
  int32_t* n_valid;
};

// the body of both entries: Q is n_feat x Sq, R is n_feat x Sr
int cross_src(icikt_ctx* c, const MatrixSrc& Q, const MatrixSrc& R, int64_t n_feat, int64_t Sq, int64_t Sr, const CrossArgs& A) {
  if (!c) return ICIKT_E_INVALID;
  icikt::host::SelectCall call{c, "cross", Q, n_feat, Sq, A.shared, {}};
  int rc = icikt::host::check_src(c, "cross (query)", Q, n_feat, Sq);
  if (!rc) rc = icikt::host::check_src(c, "cross (reference)", R, n_feat, Sr);
  if (rc) return rc;
  const int64_t ref0 = icikt::host::rect_ref_col(Sq), S_dev = ref0 + Sr;
  if (S_dev > ICIKT_TOPK_MAX_SAMPLES)
    return fail(c, ICIKT_E_INVALID, "cross: n_query + n_reference (+ 1 padding column when n_query is odd) exceeds "
                                    "ICIKT_TOPK_MAX_SAMPLES (65535 columns: the pairs of a block are indexed in 32 bits)");
  const bool want_topk = A.idx || A.out5k || A.n_valid;
  if (!A.out5 && !want_topk && !A.shared.max_taumax && !A.shared.reason_counts)
    return fail(c, ICIKT_E_INVALID, "cross: all outputs are null");
  if (want_topk && (A.k < 1 || A.k > ICIKT_TOPK_MAX))
    return fail(c, ICIKT_E_INVALID, "cross: k must be in 1 .. ICIKT_TOPK_MAX (256)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;
  const size_t k = want_topk ? (size_t)A.k : 0, SK = (size_t)Sq * k;
  if (Sq == 0 || Sr == 0) {
    // no pair: the matrices are empty, every list is padding
    const double NA = icikt::host::from_bits(icikt::host::R_NA_BITS);
    for (size_t t = 0; A.idx && t < SK; ++t) A.idx[t] = -1;
    for (size_t t = 0; A.out5k && t < 5 * SK; ++t) A.out5k[t] = NA;
    for (int64_t q = 0; A.n_valid && q < Sq; ++q) A.n_valid[q] = 0;
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const size_t P = (size_t)Sq * (size_t)Sr;
  PairBlocks blocks = PairBlocks::rect(Sq, Sr, budget);
  auto& cx = c->cross;
  if (A.out5) HIPCHK(c, cx.planes.reserve(5 * P));
  if (want_topk) {
    HIPCHK(c, cx.idx.reserve(SK));
    HIPCHK(c, cx.out.reserve(5 * SK));
    HIPCHK(c, cx.n_valid.reserve((size_t)Sq));
  }
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.upload = [&]() -> int {
    // d_X for all columns BEFORE the first upload: a DevBuf that grows drops what it holds
    HIPCHK(c, c->d_X.reserve((size_t)std::max<int64_t>(n_feat * S_dev, 1)));
    int r = icikt::host::prepare_alloc(c, n_feat, S_dev, S_dev, S_dev);
    if (r) return r;
    c->k0_mask = &call.ms;
    c->k0_keep = nullptr;
    r = icikt::host::upload_and_prepare(c, Q, n_feat, Sq, 0, Sq, flags);
    if (r) return r;
    if (ref0 > Sq) {   // the padding column: all missing, pre-passed like any column, in no pair
      r = icikt::host::timer_begin(c, ICIKT_K_PREPARE, flags);
      if (r) return r;
      HIPCHK(c, icikt::launch_cross_pad(c->d_X.p + (size_t)Sq * (size_t)n_feat, (int)n_feat, c->stream));
      r = icikt::host::prepare_launch(c, c->d_X.p, n_feat, Sq, ref0);
      if (!r) r = icikt::host::timer_end(c, ICIKT_K_PREPARE, flags);
      if (r) return r;
    }
    MatrixSrc ref = R;
    ref.dst_col = ref0;
    return icikt::host::upload_and_prepare(c, ref, n_feat, Sr, 0, Sr, flags);
  };
  steps.start = []() -> int { return ICIKT_SUCCESS; };
  steps.fold = [&](const icikt::host::PairBlock& b) -> int {
    if (want_topk)
      HIPCHK(c, icikt::launch_cross_topk(c->d_out4.p, (int)Sr, (int)k, b.row_first, b.row_last - b.row_first, (long long)Sq,
                                         cx.idx.p, cx.out.p, cx.n_valid.p, c->stream));
    if (A.out5) HIPCHK(c, icikt::launch_cross_planes(c->d_out4.p, b.count, b.begin, (long long)P, cx.planes.p, c->stream));
    return ICIKT_SUCCESS;
  };
  steps.finish = [&](unsigned long long* red) -> int {
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    const int scale = A.scale_max ? 1 : 0;
    if (want_topk) HIPCHK(c, icikt::launch_cross_cor(c->d_red.p, scale, cx.idx.p, (long long)SK, cx.out.p, c->stream));
    if (A.out5) HIPCHK(c, icikt::launch_cross_cor(c->d_red.p, scale, nullptr, (long long)P, cx.planes.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (!r && A.idx) r = icikt::host::download(c, A.idx, cx.idx.p, SK * sizeof(int32_t));
    if (!r && A.out5k) r = icikt::host::download(c, A.out5k, cx.out.p, 5 * SK * sizeof(double));
    if (!r && A.n_valid) r = icikt::host::download(c, A.n_valid, cx.n_valid.p, (size_t)Sq * sizeof(int32_t));
    if (!r && A.out5) r = icikt::host::download(c, A.out5, cx.planes.p, 5 * P * sizeof(double));
    if (!r) r = icikt::host::select_download_red(c, red);
    return r;
  };
  return icikt::host::select_run(call, blocks, steps);
}

}  // namespace

#define CROSS_ARGS CrossArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                             k, scale_max, out5, idx, out5k, n_valid}

extern "C" {

int icikt_cross_f64(icikt_ctx* c, const double* Q, int64_t ld_query, const double* R, int64_t ld_reference, int64_t n_feat,
                    int64_t n_query, int64_t n_reference, const double* global_na, int n_global_na, int k, int perspective,
                    int alternative, int continuity, uint32_t flags, int scale_max, double* out5, int32_t* idx,
                    double* out5k, int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  const icikt_input q = icikt::host::f64_view(Q, ld_query), r = icikt::host::f64_view(R, ld_reference);
  return cross_src(c, MatrixSrc::dense(&q), MatrixSrc::dense(&r), n_feat, n_query, n_reference, CROSS_ARGS);
}

int icikt_cross_in(icikt_ctx* c, const icikt_input* Q, const icikt_input* R, int64_t n_feat, int64_t n_query,
                   int64_t n_reference, const double* global_na, int n_global_na, int k, int perspective, int alternative,
                   int continuity, uint32_t flags, int scale_max, double* out5, int32_t* idx, double* out5k,
                   int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return cross_src(c, MatrixSrc::dense(Q), MatrixSrc::dense(R), n_feat, n_query, n_reference, CROSS_ARGS);
}

}  // extern "C"
