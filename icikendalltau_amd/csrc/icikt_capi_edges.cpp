// icikt_capi_edges.cpp -- host side of icikt_edges_f64 / _in / _csc: every pair i < j whose raw, p-value and completeness
// pass a rule, in combn order, compacted on the device (icikt_edges.hip).  Nothing of size S^2 is allocated: the combn
// triangle runs through the pair engine in blocks of whole rows, as icikt_topk_* runs it (select_run, icikt_host.h), and
// each block's matching records are appended to the kept planes before the next block overwrites them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct EdgeArgs {
  icikt::host::SelectArgs shared;
  const icikt_edge_rule* rule;
  int scale_max;
  int64_t max_edges;
  int32_t *ei, *ej;
  double* out5e;
  int64_t *n_edges, *degree;
};

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int edges_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const EdgeArgs& A) {
  icikt::host::SelectCall call{c, "edges", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits");
  if (rc) return rc;
  if (!A.rule) return fail(c, ICIKT_E_INVALID, "edges: null rule");
  if (A.max_edges < 0) return fail(c, ICIKT_E_INVALID, "edges: max_edges must not be negative");
  if (A.max_edges > 0 && !A.ei) return fail(c, ICIKT_E_INVALID, "edges: null output (ei)");
  if (A.max_edges > 0 && !A.ej) return fail(c, ICIKT_E_INVALID, "edges: null output (ej)");
  if (A.max_edges > 0 && !A.out5e) return fail(c, ICIKT_E_INVALID, "edges: null output (out5e)");
  if (!A.n_edges) return fail(c, ICIKT_E_INVALID, "edges: null output (n_edges)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;
  *A.n_edges = 0;
  if (A.degree) for (int64_t s = 0; s < n_samp; ++s) A.degree[s] = 0;
  if (n_samp == 0) return ICIKT_SUCCESS;
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const uint32_t flags = A.shared.flags;
  const int64_t S = n_samp;
  PairBlocks blocks = PairBlocks::rows(S, budget);
  const int64_t cap = std::min(A.max_edges, blocks.total);   // slots of the kept planes on the device
  const size_t tiles_max = (size_t)icikt::edge_tiles(blocks.block_max);
  auto& ed = c->edges;
  HIPCHK(c, ed.ballots.reserve(tiles_max * icikt::EDGE_TILE_WORDS));
  HIPCHK(c, ed.counts.reserve(tiles_max));
  HIPCHK(c, ed.bases.reserve(tiles_max));
  HIPCHK(c, ed.total.reserve(1));
  HIPCHK(c, ed.degree.reserve((size_t)S));
  HIPCHK(c, ed.ei.reserve((size_t)cap));
  HIPCHK(c, ed.ej.reserve((size_t)cap));
  HIPCHK(c, ed.vals.reserve(5 * (size_t)cap));
  icikt::EdgeOut E{};
  if (cap > 0)
    E = icikt::EdgeOut{ed.ei.p, ed.ej.p, ed.vals.p, ed.vals.p + cap, ed.vals.p + 2 * cap, ed.vals.p + 3 * cap,
                       ed.vals.p + 4 * cap, (long long)cap};
  const icikt::EdgeRule R{A.rule->min_raw, A.rule->max_pvalue, A.rule->min_completeness, A.rule->absolute ? 1 : 0};
  unsigned long long* const d_degree = A.degree ? ed.degree.p : nullptr;
  unsigned long long n_match = 0;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(ed.total.p, 0, sizeof(unsigned long long), c->stream));
    if (d_degree) HIPCHK(c, hipMemsetAsync(d_degree, 0, (size_t)S * sizeof(unsigned long long), c->stream));
    return ICIKT_SUCCESS;
  };
  steps.fold = [&](const icikt::host::PairBlock& b) -> int {
    HIPCHK(c, icikt::launch_edge_block(R, c->d_out4.p, b.count, b.begin, (int)S, ed.ballots.p, ed.counts.p, ed.bases.p,
                                       ed.total.p, d_degree, E, c->stream));
    return ICIKT_SUCCESS;
  };
  steps.finish = [&](unsigned long long* red) -> int {
    // the count decides how much there is to finish and to bring back: the one wait inside the call
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&n_match, ed.total.p, sizeof(n_match), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t n_kept = (int64_t)std::min<unsigned long long>(n_match, (unsigned long long)cap);
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_edge_finish(E, n_kept, c->d_red.p, A.scale_max ? 1 : 0, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    r = icikt::host::download(c, A.ei, ed.ei.p, (size_t)n_kept * sizeof(int32_t));
    if (!r) r = icikt::host::download(c, A.ej, ed.ej.p, (size_t)n_kept * sizeof(int32_t));
    for (int q = 0; q < 5 && !r; ++q)   // the caller's planes are max_edges apart, the device's cap
      r = icikt::host::download(c, A.out5e + (size_t)q * (size_t)A.max_edges, ed.vals.p + (size_t)q * (size_t)cap,
                                (size_t)n_kept * sizeof(double));
    if (!r && A.degree) r = icikt::host::download(c, A.degree, ed.degree.p, (size_t)S * sizeof(int64_t));
    return r;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) *A.n_edges = (int64_t)n_match;
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define EDGE_ARGS EdgeArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                           rule, scale_max, max_edges, ei, ej, out5e, n_edges, degree}

extern "C" {

int icikt_edges_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                    int n_global_na, const icikt_edge_rule* rule, int perspective, int alternative, int continuity,
                    uint32_t flags, int scale_max, int64_t max_edges, int32_t* ei, int32_t* ej, double* out5e,
                    int64_t* n_edges, int64_t* degree, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return edges_src(c, MatrixSrc::dense(&v), n_feat, n_samp, EDGE_ARGS);
}

int icikt_edges_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, const icikt_edge_rule* rule, int perspective, int alternative, int continuity,
                   uint32_t flags, int scale_max, int64_t max_edges, int32_t* ei, int32_t* ej, double* out5e,
                   int64_t* n_edges, int64_t* degree, double* max_taumax, int64_t* reason_counts) {
  return edges_src(c, MatrixSrc::dense(X), n_feat, n_samp, EDGE_ARGS);
}

int icikt_edges_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, const icikt_edge_rule* rule, int perspective, int alternative, int continuity,
                    uint32_t flags, int scale_max, int64_t max_edges, int32_t* ei, int32_t* ej, double* out5e,
                    int64_t* n_edges, int64_t* degree, double* max_taumax, int64_t* reason_counts) {
  return edges_src(c, MatrixSrc::csc(X), n_feat, n_samp, EDGE_ARGS);
}

}  // extern "C"
