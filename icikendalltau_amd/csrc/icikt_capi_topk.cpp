// icikt_capi_topk.cpp -- host side of icikt_topk_f64 / _in / _csc: every sample's k partners with the largest
// ICI-Kendall-tau, selected on the device (icikt_topk.hip).  Nothing of size S^2 is allocated: the combn triangle runs
// through the pair engine in blocks of whole rows, and each block's records are folded into the columns' lists before
// the next block overwrites them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::timer_begin;
using icikt::host::timer_end;

using icikt::host::cut_rows;
using icikt::host::row_offset;

namespace {

// the body of the three entries (the block cut: cut_rows, icikt_host.h)
int topk_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na, int n_global_na,
             int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max, int32_t* idx,
             double* out5k, int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  if (!c) return ICIKT_E_INVALID;
  // every argument is validated before anything of the context is touched
  int rc = icikt::host::check_src(c, "topk", X, n_feat, n_samp);
  if (rc) return rc;
  if (n_samp > ICIKT_TOPK_MAX_SAMPLES)
    return fail(c, ICIKT_E_INVALID, "topk: n_samp exceeds ICIKT_TOPK_MAX_SAMPLES (65535 samples: the pairs of the triangle are indexed in 32 bits)");
  if (k < 1 || k > ICIKT_TOPK_MAX) return fail(c, ICIKT_E_INVALID, "topk: k must be in 1 .. ICIKT_TOPK_MAX (256)");
  if (n_samp > 0 && !idx) return fail(c, ICIKT_E_INVALID, "topk: null output (idx)");
  if (n_samp > 0 && !out5k) return fail(c, ICIKT_E_INVALID, "topk: null output (out5k)");
  if (perspective != ICIKT_PERSPECTIVE_LOCAL && perspective != ICIKT_PERSPECTIVE_GLOBAL)
    return fail(c, ICIKT_E_INVALID, "topk: perspective must be local (0) or global (1)");
  if (alternative < 0 || alternative > ICIKT_ALT_OTHER) return fail(c, ICIKT_E_INVALID, "topk: bad alternative code");
  icikt::MaskSpec ms;
  rc = icikt::host::make_mask_spec(c, global_na, n_global_na, &ms);
  if (rc) return rc;
  if (reason_counts) for (int r = 0; r < 5; ++r) reason_counts[r] = 0;
  if (max_taumax) *max_taumax = -HUGE_VAL;   // max(numeric(0), na.rm = TRUE)
  if (n_samp == 0) return ICIKT_SUCCESS;
  rc = icikt::host::use_device(c);
  if (rc) return rc;

  const int64_t S = n_samp, total = S * (S - 1) / 2;
  const size_t SK = (size_t)S * (size_t)k;
  const int64_t budget = c->plan_ov.tkblock > 0 ? c->plan_ov.tkblock : icikt::host::kTriangleBlockPairs;
  const std::vector<std::pair<int, int>> blocks = cut_rows(S, budget);
  int64_t block_max = 1;
  for (const auto& b : blocks) block_max = std::max(block_max, row_offset(S, b.second) - row_offset(S, b.first));

  auto& tk = c->topk;
  HIPCHK(c, tk.key.reserve(2 * SK));
  HIPCHK(c, tk.partner.reserve(2 * SK));
  HIPCHK(c, tk.vals.reserve(8 * SK));
  HIPCHK(c, tk.state.reserve(2 * (size_t)S));
  HIPCHK(c, tk.idx.reserve(SK));
  HIPCHK(c, tk.out.reserve(5 * SK));
  HIPCHK(c, tk.n_valid.reserve((size_t)S));
  HIPCHK(c, c->d_red.reserve(8));
  const icikt::TopkLists L{tk.key.p, tk.partner.p, tk.vals.p, tk.state.p, tk.state.p + S, k};

  // from here on the context holds this call's scratch state and nothing of the caller's: whatever happens, the
  // device-resident calls start over afterwards (icikt_run_dev: ICIKT_E_STATE, icikt_num_pairs: -1)
  auto leave = [c](int r) {
    r = icikt::host::end_call(c, "topk", r);
    c->prepared = false;
    c->raw_valid = false;
    c->n_pairs = -1;
    c->pairs_nsamp = -1;
    c->wpb = 0;
    c->combn_S = -1;
    return r;
  };
  const icikt::host::PinnedScope scope(c, flags);
  const uint32_t run_flags = flags & ~(uint32_t)ICIKT_FLAG_REUSE_COUNTS;
  unsigned long long red[8] = {};
  auto body = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(tk.state.p, 0, 2 * (size_t)S * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_red.p, 0, 8 * sizeof(unsigned long long), c->stream));
    if (!blocks.empty()) {
      HIPCHK(c, c->d_out4.reserve((size_t)block_max * 4));
      HIPCHK(c, c->d_reasons.reserve((size_t)block_max));
      // a triangle that is one block takes the matrix entries' way in: copies, pre-pass and pair kernel pipelined by
      // column chunks (upload_prepare_pairs); several blocks: the matrix first, then block after block
      const bool one = blocks.size() == 1;
      int r = one ? icikt_set_pairs_combn(c, S, 0, total) : ICIKT_SUCCESS;
      if (r) return r;
      r = icikt::host::prepare_alloc(c, n_feat, n_samp, n_samp, n_samp);
      if (r) return r;
      c->k0_mask = &ms;
      c->k0_keep = nullptr;
      r = one ? icikt::host::upload_prepare_pairs(c, X, n_feat, n_samp, flags)
              : icikt::host::upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags);
      c->k0_mask = nullptr;
      if (r) return r;
      c->prepared = true;
      for (const auto& b : blocks) {
        const int64_t begin = row_offset(S, b.first), end = row_offset(S, b.second);
        if (!one) {
          r = icikt_set_pairs_combn(c, S, begin, end);
          if (r) return r;
        }
        r = icikt_run_dev(c, perspective, alternative, continuity,
                          run_flags | ((one && c->raw_valid) ? ICIKT_FLAG_REUSE_COUNTS : 0u), c->d_out4.p, nullptr,
                          c->d_reasons.p);
        if (r) return r;
        r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
        if (r) return r;
        HIPCHK(c, icikt::launch_out_stats_accum(c->pv, c->d_out4.p, c->d_reasons.p, end - begin, c->d_red.p, c->stream));
        HIPCHK(c, icikt::launch_topk_merge(L, c->d_out4.p, (int)S, b.first, b.second, c->stream));
        r = timer_end(c, ICIKT_K_EPILOGUE, flags);
        if (r) return r;
      }
    }
    int r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_topk_finish(L, c->d_red.p, (int)S, scale_max ? 1 : 0, tk.idx.p, tk.out.p, tk.n_valid.p, c->stream));
    r = timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, idx, tk.idx.p, SK * sizeof(int32_t));
    if (!r) r = icikt::host::download(c, out5k, tk.out.p, 5 * SK * sizeof(double));
    if (!r && n_valid) r = icikt::host::download(c, n_valid, tk.n_valid.p, (size_t)S * sizeof(int32_t));
    if (!r) r = icikt::host::download(c, red, c->d_red.p, sizeof(red));
    return r;
  };
  rc = leave(body());
  c->k0_mask = nullptr;
  if (rc) return rc;
  if (reason_counts) for (int r = 0; r < 5; ++r) reason_counts[r] = (int64_t)red[1 + r];
  if (max_taumax && red[0]) {
    const unsigned long long u = (red[0] >> 63) ? (red[0] & 0x7FFFFFFFFFFFFFFFull) : ~red[0];
    std::memcpy(max_taumax, &u, sizeof(double));
  }
  return ICIKT_SUCCESS;
}

}  // namespace

extern "C" {

int icikt_topk_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                   int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags,
                   int scale_max, int32_t* idx, double* out5k, int32_t* n_valid, double* max_taumax,
                   int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return topk_src(c, MatrixSrc::dense(&v), n_feat, n_samp, global_na, n_global_na, k, perspective, alternative,
                  continuity, flags, scale_max, idx, out5k, n_valid, max_taumax, reason_counts);
}

int icikt_topk_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                  int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  int32_t* idx, double* out5k, int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return topk_src(c, MatrixSrc::dense(X), n_feat, n_samp, global_na, n_global_na, k, perspective, alternative, continuity,
                  flags, scale_max, idx, out5k, n_valid, max_taumax, reason_counts);
}

int icikt_topk_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                   int32_t* idx, double* out5k, int32_t* n_valid, double* max_taumax, int64_t* reason_counts) {
  return topk_src(c, MatrixSrc::csc(X), n_feat, n_samp, global_na, n_global_na, k, perspective, alternative, continuity,
                  flags, scale_max, idx, out5k, n_valid, max_taumax, reason_counts);
}

}  // extern "C"
