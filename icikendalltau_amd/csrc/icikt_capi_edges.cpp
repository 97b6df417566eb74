// icikt_capi_edges.cpp -- host side of icikt_edges_f64 / _in / _csc: every pair i < j whose raw, p-value and completeness
// pass a rule, in combn order, compacted on the device (icikt_edges.hip).  Nothing of size S^2 is allocated: the combn
// triangle runs through the pair engine in blocks of whole rows, as icikt_topk_* runs it (cut_rows, icikt_host.h), and
// each block's matching records are appended to the kept planes before the next block overwrites them.
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

using icikt::host::cut_rows;
using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::row_offset;
using icikt::host::timer_begin;
using icikt::host::timer_end;

namespace {

struct EdgeArgs {
  const double* global_na;
  int n_global_na;
  const icikt_edge_rule* rule;
  int perspective, alternative, continuity;
  uint32_t flags;
  int scale_max;
  int64_t max_edges;
  int32_t *ei, *ej;
  double* out5e;
  int64_t *n_edges, *degree;
  double* max_taumax;
  int64_t* reason_counts;
};

// the body of the three entries
int edges_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const EdgeArgs& A) {
  if (!c) return ICIKT_E_INVALID;
  // every argument is validated before anything of the context, or any output, is touched
  int rc = icikt::host::check_src(c, "edges", X, n_feat, n_samp);
  if (rc) return rc;
  if (n_samp > ICIKT_TOPK_MAX_SAMPLES)
    return fail(c, ICIKT_E_INVALID, "edges: n_samp exceeds ICIKT_TOPK_MAX_SAMPLES (65535 samples: the pairs of the triangle are indexed in 32 bits)");
  if (!A.rule) return fail(c, ICIKT_E_INVALID, "edges: null rule");
  if (A.max_edges < 0) return fail(c, ICIKT_E_INVALID, "edges: max_edges must not be negative");
  if (A.max_edges > 0 && !A.ei) return fail(c, ICIKT_E_INVALID, "edges: null output (ei)");
  if (A.max_edges > 0 && !A.ej) return fail(c, ICIKT_E_INVALID, "edges: null output (ej)");
  if (A.max_edges > 0 && !A.out5e) return fail(c, ICIKT_E_INVALID, "edges: null output (out5e)");
  if (!A.n_edges) return fail(c, ICIKT_E_INVALID, "edges: null output (n_edges)");
  if (A.perspective != ICIKT_PERSPECTIVE_LOCAL && A.perspective != ICIKT_PERSPECTIVE_GLOBAL)
    return fail(c, ICIKT_E_INVALID, "edges: perspective must be local (0) or global (1)");
  if (A.alternative < 0 || A.alternative > ICIKT_ALT_OTHER) return fail(c, ICIKT_E_INVALID, "edges: bad alternative code");
  icikt::MaskSpec ms;
  rc = icikt::host::make_mask_spec(c, A.global_na, A.n_global_na, &ms);
  if (rc) return rc;
  *A.n_edges = 0;
  if (A.degree) for (int64_t s = 0; s < n_samp; ++s) A.degree[s] = 0;
  if (A.reason_counts) for (int r = 0; r < 5; ++r) A.reason_counts[r] = 0;
  if (A.max_taumax) *A.max_taumax = -HUGE_VAL;   // max(numeric(0), na.rm = TRUE)
  if (n_samp == 0) return ICIKT_SUCCESS;
  rc = icikt::host::use_device(c);
  if (rc) return rc;

  const uint32_t flags = A.flags;
  const int64_t S = n_samp, total = S * (S - 1) / 2;
  const int64_t cap = std::min(A.max_edges, total);   // slots of the kept planes on the device
  const int64_t budget = c->plan_ov.tkblock > 0 ? c->plan_ov.tkblock : icikt::host::kTriangleBlockPairs;
  const std::vector<std::pair<int, int>> blocks = cut_rows(S, budget);
  int64_t block_max = 1;
  for (const auto& b : blocks) block_max = std::max(block_max, row_offset(S, b.second) - row_offset(S, b.first));
  const size_t tiles_max = (size_t)icikt::edge_tiles(block_max);

  auto& ed = c->edges;
  HIPCHK(c, ed.ballots.reserve(tiles_max * icikt::EDGE_TILE_WORDS));
  HIPCHK(c, ed.counts.reserve(tiles_max));
  HIPCHK(c, ed.bases.reserve(tiles_max));
  HIPCHK(c, ed.total.reserve(1));
  HIPCHK(c, ed.degree.reserve((size_t)S));
  HIPCHK(c, ed.ei.reserve((size_t)cap));
  HIPCHK(c, ed.ej.reserve((size_t)cap));
  HIPCHK(c, ed.vals.reserve(5 * (size_t)cap));
  HIPCHK(c, c->d_red.reserve(8));
  icikt::EdgeOut E{};
  if (cap > 0)
    E = icikt::EdgeOut{ed.ei.p, ed.ej.p, ed.vals.p, ed.vals.p + cap, ed.vals.p + 2 * cap, ed.vals.p + 3 * cap,
                       ed.vals.p + 4 * cap, (long long)cap};
  const icikt::EdgeRule R{A.rule->min_raw, A.rule->max_pvalue, A.rule->min_completeness, A.rule->absolute ? 1 : 0};
  unsigned long long* const d_degree = A.degree ? ed.degree.p : nullptr;

  // from here on the context holds this call's scratch state and nothing of the caller's: whatever happens, the
  // device-resident calls start over afterwards (icikt_run_dev: ICIKT_E_STATE, icikt_num_pairs: -1)
  auto leave = [c](int r) {
    r = icikt::host::end_call(c, "edges", r);
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
  unsigned long long n_match = 0;
  auto body = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(ed.total.p, 0, sizeof(unsigned long long), c->stream));
    if (d_degree) HIPCHK(c, hipMemsetAsync(d_degree, 0, (size_t)S * sizeof(unsigned long long), c->stream));
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
        r = icikt_run_dev(c, A.perspective, A.alternative, A.continuity,
                          run_flags | ((one && c->raw_valid) ? ICIKT_FLAG_REUSE_COUNTS : 0u), c->d_out4.p, nullptr,
                          c->d_reasons.p);
        if (r) return r;
        r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
        if (r) return r;
        HIPCHK(c, icikt::launch_out_stats_accum(c->pv, c->d_out4.p, c->d_reasons.p, end - begin, c->d_red.p, c->stream));
        HIPCHK(c, icikt::launch_edge_block(R, c->d_out4.p, end - begin, begin, (int)S, ed.ballots.p, ed.counts.p,
                                           ed.bases.p, ed.total.p, d_degree, E, c->stream));
        r = timer_end(c, ICIKT_K_EPILOGUE, flags);
        if (r) return r;
      }
    }
    // the count decides how much there is to finish and to bring back: the one wait inside the call
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, sizeof(red), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&n_match, ed.total.p, sizeof(n_match), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t n_kept = (int64_t)std::min<unsigned long long>(n_match, (unsigned long long)cap);
    int r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_edge_finish(E, n_kept, c->d_red.p, A.scale_max ? 1 : 0, c->stream));
    r = timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, A.ei, ed.ei.p, (size_t)n_kept * sizeof(int32_t));
    if (!r) r = icikt::host::download(c, A.ej, ed.ej.p, (size_t)n_kept * sizeof(int32_t));
    for (int q = 0; q < 5 && !r; ++q)   // the caller's planes are max_edges apart, the device's cap
      r = icikt::host::download(c, A.out5e + (size_t)q * (size_t)A.max_edges, ed.vals.p + (size_t)q * (size_t)cap,
                                (size_t)n_kept * sizeof(double));
    if (!r && A.degree) r = icikt::host::download(c, A.degree, ed.degree.p, (size_t)S * sizeof(int64_t));
    return r;
  };
  rc = leave(body());
  c->k0_mask = nullptr;
  if (rc) return rc;
  *A.n_edges = (int64_t)n_match;
  if (A.reason_counts) for (int r = 0; r < 5; ++r) A.reason_counts[r] = (int64_t)red[1 + r];
  if (A.max_taumax && red[0]) {
    const unsigned long long u = (red[0] >> 63) ? (red[0] & 0x7FFFFFFFFFFFFFFFull) : ~red[0];
    std::memcpy(A.max_taumax, &u, sizeof(double));
  }
  return ICIKT_SUCCESS;
}

}  // namespace

extern "C" {

int icikt_edges_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                    int n_global_na, const icikt_edge_rule* rule, int perspective, int alternative, int continuity,
                    uint32_t flags, int scale_max, int64_t max_edges, int32_t* ei, int32_t* ej, double* out5e,
                    int64_t* n_edges, int64_t* degree, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return edges_src(c, MatrixSrc::dense(&v), n_feat, n_samp,
                   EdgeArgs{global_na, n_global_na, rule, perspective, alternative, continuity, flags, scale_max, max_edges,
                            ei, ej, out5e, n_edges, degree, max_taumax, reason_counts});
}

int icikt_edges_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, const icikt_edge_rule* rule, int perspective, int alternative, int continuity,
                   uint32_t flags, int scale_max, int64_t max_edges, int32_t* ei, int32_t* ej, double* out5e,
                   int64_t* n_edges, int64_t* degree, double* max_taumax, int64_t* reason_counts) {
  return edges_src(c, MatrixSrc::dense(X), n_feat, n_samp,
                   EdgeArgs{global_na, n_global_na, rule, perspective, alternative, continuity, flags, scale_max, max_edges,
                            ei, ej, out5e, n_edges, degree, max_taumax, reason_counts});
}

int icikt_edges_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, const icikt_edge_rule* rule, int perspective, int alternative, int continuity,
                    uint32_t flags, int scale_max, int64_t max_edges, int32_t* ei, int32_t* ej, double* out5e,
                    int64_t* n_edges, int64_t* degree, double* max_taumax, int64_t* reason_counts) {
  return edges_src(c, MatrixSrc::csc(X), n_feat, n_samp,
                   EdgeArgs{global_na, n_global_na, rule, perspective, alternative, continuity, flags, scale_max, max_edges,
                            ei, ej, out5e, n_edges, degree, max_taumax, reason_counts});
}

}  // extern "C"
