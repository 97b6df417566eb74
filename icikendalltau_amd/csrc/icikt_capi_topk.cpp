// icikt_capi_topk.cpp -- host side of icikt_topk_f64 / _in / _csc: every sample's k partners with the largest
// ICI-Kendall-tau, selected on the device (icikt_topk.hip).  Nothing of size S^2 is allocated: the combn triangle runs
// through the pair engine in blocks of whole rows, and each block's records are folded into the columns' lists before
// the next block overwrites them.
#include <hip/hip_runtime.h>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct TopkArgs {
  icikt::host::SelectArgs shared;
  int k, scale_max;
  int32_t* idx;
  double* out5k;
  int32_t* n_valid;
};

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int topk_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const TopkArgs& A) {
  icikt::host::SelectCall call{c, "topk", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits");
  if (rc) return rc;
  if (A.k < 1 || A.k > ICIKT_TOPK_MAX) return fail(c, ICIKT_E_INVALID, "topk: k must be in 1 .. ICIKT_TOPK_MAX (256)");
  if (n_samp > 0 && !A.idx) return fail(c, ICIKT_E_INVALID, "topk: null output (idx)");
  if (n_samp > 0 && !A.out5k) return fail(c, ICIKT_E_INVALID, "topk: null output (out5k)");
  rc = icikt::host::select_check_args(call);
  if (rc || n_samp == 0) return rc;
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const int64_t S = n_samp;
  const size_t SK = (size_t)S * (size_t)A.k;
  PairBlocks blocks = PairBlocks::rows(S, budget);
  auto& tk = c->topk;
  HIPCHK(c, tk.key.reserve(2 * SK));
  HIPCHK(c, tk.partner.reserve(2 * SK));
  HIPCHK(c, tk.vals.reserve(8 * SK));
  HIPCHK(c, tk.state.reserve(2 * (size_t)S));
  HIPCHK(c, tk.idx.reserve(SK));
  HIPCHK(c, tk.out.reserve(5 * SK));
  HIPCHK(c, tk.n_valid.reserve((size_t)S));
  const icikt::TopkLists L{tk.key.p, tk.partner.p, tk.vals.p, tk.state.p, tk.state.p + S, A.k};
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(tk.state.p, 0, 2 * (size_t)S * sizeof(int32_t), c->stream));
    return ICIKT_SUCCESS;
  };
  steps.fold = [&](const icikt::host::PairBlock& b) -> int {
    HIPCHK(c, icikt::launch_topk_merge(L, c->d_out4.p, (int)S, b.row_first, b.row_last, c->stream));
    return ICIKT_SUCCESS;
  };
  steps.finish = [&](unsigned long long* red) -> int {
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_topk_finish(L, c->d_red.p, (int)S, A.scale_max ? 1 : 0, tk.idx.p, tk.out.p, tk.n_valid.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, A.idx, tk.idx.p, SK * sizeof(int32_t));
    if (!r) r = icikt::host::download(c, A.out5k, tk.out.p, 5 * SK * sizeof(double));
    if (!r && A.n_valid) r = icikt::host::download(c, A.n_valid, tk.n_valid.p, (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::select_download_red(c, red);
    return r;
  };
  return icikt::host::select_run(call, blocks, steps);
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define TOPK_ARGS TopkArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                           k, scale_max, idx, out5k, n_valid}

extern "C" {

int icikt_topk_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                   int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags,
                   int scale_max, int32_t* idx, double* out5k, int32_t* n_valid, double* max_taumax,
                   int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return topk_src(c, MatrixSrc::dense(&v), n_feat, n_samp, TOPK_ARGS);
}

int icikt_topk_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                  int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  int32_t* idx, double* out5k, int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return topk_src(c, MatrixSrc::dense(X), n_feat, n_samp, TOPK_ARGS);
}

int icikt_topk_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                   int32_t* idx, double* out5k, int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return topk_src(c, MatrixSrc::csc(X), n_feat, n_samp, TOPK_ARGS);
}

}  // extern "C"
