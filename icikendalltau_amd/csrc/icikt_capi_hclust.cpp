// icikt_capi_hclust.cpp -- host side of icikt_hclust_f64 / _in / _csc: agglomerative clustering of the samples under raw
// with complete, average or single linkage, run on the device (icikt_hclust.hip, which states the rule in full).  The
// whole combn triangle runs through the pair engine in blocks of rows; each block's raw values are kept as sortable keys
// (8 bytes per pair, launch_median_keep) before the next block overwrites them.  After the last block k_hc_expand makes
// the symmetric S x S table of keys, one scan gives every row its best partner, and S - 1 steps of three launches each
// (k_hc_pick, k_hc_merge, k_hc_rescan) are queued on the context's stream without a host wait: a step that finds no
// pair to merge sets a device flag, and the launches behind it return at once.  Only the merge records (24 B each) and
// the state words come back, behind one wait; the host derives the components from the records and checks them in O(S).
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), 8 S (S - 1) / 2 bytes
// of kept keys in the workspace's `kept` plane (icikt_ctx::sel, shared with the other entries), 8 S^2 bytes of table -- 12 S^2 together (65 535 samples: 52 GB) -- and 40 S bytes of neighbours (4 + 8),
// live flags, sizes and list (4 each) and merge records (24, less one), each with the buffers' growth margin of a ninth.
// Host memory: O(S), never O(S^2).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
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

struct HclustArgs {
  icikt::host::SelectArgs shared;
  int scale_max, method;
  double min_raw;
  int32_t *ma, *mb, *msize;
  double *mraw, *mcor;
  int64_t* n_merges;
  int32_t* component;
  int64_t* n_components;
};

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int hclust_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const HclustArgs& A) {
  icikt::host::SelectCall call{c, "hclust", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the table of similarities is indexed by two 16-bit slots");
  if (rc) return rc;
  if (A.method != ICIKT_HCLUST_COMPLETE && A.method != ICIKT_HCLUST_AVERAGE && A.method != ICIKT_HCLUST_SINGLE)
    return fail(c, ICIKT_E_INVALID, "hclust: method must be complete (0), average (1) or single (2)");
  if (n_samp > 1 && !A.ma) return fail(c, ICIKT_E_INVALID, "hclust: null output (ma)");
  if (n_samp > 1 && !A.mb) return fail(c, ICIKT_E_INVALID, "hclust: null output (mb)");
  if (n_samp > 1 && !A.msize) return fail(c, ICIKT_E_INVALID, "hclust: null output (msize)");
  if (n_samp > 1 && !A.mraw) return fail(c, ICIKT_E_INVALID, "hclust: null output (mraw)");
  if (n_samp > 1 && !A.mcor) return fail(c, ICIKT_E_INVALID, "hclust: null output (mcor)");
  if (!A.n_merges) return fail(c, ICIKT_E_INVALID, "hclust: null output (n_merges)");
  if (n_samp > 0 && !A.component) return fail(c, ICIKT_E_INVALID, "hclust: null output (component)");
  if (!A.n_components) return fail(c, ICIKT_E_INVALID, "hclust: null output (n_components)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;
  *A.n_merges = 0;
  *A.n_components = 0;
  if (n_samp == 0) return ICIKT_SUCCESS;
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const int64_t S = n_samp;
  const uint32_t flags = A.shared.flags;
  const unsigned long long min_key = A.min_raw == A.min_raw ? icikt::host::cor_key(A.min_raw) : 0ull;   // NaN: no bound
  const int grid = c->plan_ov.hcgrid > 0 ? c->plan_ov.hcgrid : (int)std::min<int64_t>(S, icikt::HCLUST_GRID_MAX);
  PairBlocks blocks = PairBlocks::rows(S, budget);
  auto& hb = c->hc;
  HIPCHK(c, c->sel.kept.reserve((size_t)std::max<int64_t>(blocks.total, 1)));
  HIPCHK(c, hb.table.reserve((size_t)S * (size_t)S));
  HIPCHK(c, hb.nnkey.reserve((size_t)S));
  HIPCHK(c, hb.nn.reserve((size_t)S));
  HIPCHK(c, hb.alive.reserve((size_t)S));
  HIPCHK(c, hb.size.reserve((size_t)S));
  HIPCHK(c, hb.list.reserve((size_t)S));
  HIPCHK(c, hb.state.reserve((size_t)icikt::HC_WORDS));
  HIPCHK(c, hb.rec.reserve((size_t)std::max<int64_t>(S - 1, 1)));

  std::vector<icikt::HcMerge> rec;
  std::vector<int32_t> comp, root, live, size;
  int64_t n_merges = 0, n_comp = 0;
  unsigned long long red0 = 0ull;   // word 0 of launch_out_stats' record: the largest taumax as a key (0: no pair had one)

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int { return ICIKT_SUCCESS; };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    int32_t state[icikt::HC_WORDS] = {};
    try {
      rec.resize((size_t)(S - 1));
      comp.resize((size_t)S);
      root.resize((size_t)S);
      live.assign((size_t)S, 1);
      size.assign((size_t)S, 1);
    } catch (const std::bad_alloc&) {
      return fail(c, ICIKT_E_NOMEM, "hclust: host allocation failed");
    }
    if (S > 1) {
      // ---- the table, the first neighbours and S - 1 steps, queued without a wait: 2 + 3 (S - 1) launches ----
      int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
      if (r) return r;
      HIPCHK(c, hipMemsetAsync(hb.state.p, 0, icikt::HC_WORDS * sizeof(int32_t), c->stream));
      HIPCHK(c, icikt::launch_hc_expand(c->sel.kept.p, (int)S, hb.table.p, hb.alive.p, hb.size.p, c->stream));
      HIPCHK(c, icikt::launch_hc_rescan(hb.table.p, hb.alive.p, hb.list.p, hb.state.p, (int)S, 1, grid, hb.nn.p,
                                        hb.nnkey.p, c->stream));
      for (int64_t t = 0; t < S - 1; ++t) {
        HIPCHK(c, icikt::launch_hc_pick(hb.nn.p, hb.nnkey.p, hb.alive.p, hb.size.p, hb.state.p, hb.rec.p, min_key,
                                        (int)S, c->stream));
        HIPCHK(c, icikt::launch_hc_merge(hb.table.p, hb.nn.p, hb.nnkey.p, hb.alive.p, hb.list.p, hb.state.p, A.method,
                                         (int)S, c->stream));
        HIPCHK(c, icikt::launch_hc_rescan(hb.table.p, hb.alive.p, hb.list.p, hb.state.p, (int)S, 0, grid, hb.nn.p,
                                          hb.nnkey.p, c->stream));
      }
      r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
      if (r) return r;
      HIPCHK(c, hipMemcpyAsync(rec.data(), hb.rec.p, (size_t)(S - 1) * sizeof(icikt::HcMerge), hipMemcpyDeviceToHost,
                               c->stream));
      HIPCHK(c, hipMemcpyAsync(state, hb.state.p, sizeof state, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    red0 = red[0];
    // ---- the records, checked in one pass: only the first n_merges were written by this call ----
    n_merges = state[icikt::HC_MERGES];
    if (n_merges < 0 || n_merges > S - 1)
      return fail(c, ICIKT_E_STATE, "hclust: the device counted " + std::to_string(n_merges) + " merges of " +
                                        std::to_string(S) + " samples");
    if (!state[icikt::HC_DONE] && n_merges != S - 1)
      return fail(c, ICIKT_E_STATE, "hclust: the steps ended neither in one cluster nor at a step without a pair to merge");
    for (int64_t s = 0; s < S; ++s) root[(size_t)s] = (int32_t)s;
    const bool monotone = A.method != ICIKT_HCLUST_AVERAGE;   // a minimum or maximum of keys never exceeds the step's best
    for (int64_t t = 0; t < n_merges; ++t) {
      const icikt::HcMerge& m = rec[(size_t)t];
      const std::string at = "hclust: merge " + std::to_string(t);
      if (m.a < 0 || m.b >= S || m.a >= m.b)
        return fail(c, ICIKT_E_STATE, at + " names the slots " + std::to_string(m.a) + ", " + std::to_string(m.b));
      if (!live[(size_t)m.a] || !live[(size_t)m.b]) return fail(c, ICIKT_E_STATE, at + " names a slot that is no cluster any more");
      if (m.key == 0ull || m.key == icikt::host::NA_KEY) return fail(c, ICIKT_E_STATE, at + " has no similarity");
      if (m.key < min_key) return fail(c, ICIKT_E_STATE, at + " lies below min_raw");
      if (m.size != size[(size_t)m.a] + size[(size_t)m.b]) return fail(c, ICIKT_E_STATE, at + " has another size than its two clusters");
      if (monotone && t > 0 && m.key > rec[(size_t)(t - 1)].key)
        return fail(c, ICIKT_E_STATE, at + " is better than the merge before it: not the strict order");
      live[(size_t)m.b] = 0;
      size[(size_t)m.a] = m.size;
      root[(size_t)m.b] = m.a;
    }
    // ---- components, numbered in order of their smallest sample: a slot merges into a smaller one, so its cluster's
    // slot is known once the smaller slots' are ----
    n_comp = 0;
    for (int64_t s = 0; s < S; ++s) {
      if (root[(size_t)s] == s) comp[(size_t)s] = (int32_t)n_comp++;
      else { root[(size_t)s] = root[(size_t)root[(size_t)s]]; comp[(size_t)s] = comp[(size_t)root[(size_t)s]]; }
    }
    if (n_merges + n_comp != S)
      return fail(c, ICIKT_E_STATE, "hclust: " + std::to_string(n_merges) + " merges and " + std::to_string(n_comp) +
                                        " components do not add up to " + std::to_string(S) + " samples");
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (rc) return rc;

  // the outputs, once nothing can fail any more; the slots behind n_merges stay untouched
  const double max_cor = icikt::host::max_taumax_of(red0);
  for (int64_t t = 0; t < n_merges; ++t) {
    const icikt::HcMerge& m = rec[(size_t)t];
    const double raw = icikt::host::cor_key_value(m.key);
    A.ma[t] = m.a;
    A.mb[t] = m.b;
    A.msize[t] = m.size;
    A.mraw[t] = raw;
    A.mcor[t] = A.scale_max ? raw / max_cor : raw;   // k_assemble's expression
  }
  for (int64_t s = 0; s < S; ++s) A.component[s] = comp[(size_t)s];
  *A.n_merges = n_merges;
  *A.n_components = n_comp;
  return ICIKT_SUCCESS;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define HCLUST_ARGS HclustArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                               scale_max, method, min_raw, ma, mb, msize, mraw, mcor, n_merges, component, n_components}

extern "C" {

int icikt_hclust_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                     int method, double min_raw, int32_t* ma, int32_t* mb, int32_t* msize, double* mraw, double* mcor,
                     int64_t* n_merges, int32_t* component, int64_t* n_components, double* max_taumax,
                     int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return hclust_src(c, MatrixSrc::dense(&v), n_feat, n_samp, HCLUST_ARGS);
}

int icikt_hclust_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                    int method, double min_raw, int32_t* ma, int32_t* mb, int32_t* msize, double* mraw, double* mcor,
                    int64_t* n_merges, int32_t* component, int64_t* n_components, double* max_taumax,
                    int64_t* reason_counts) {
  return hclust_src(c, MatrixSrc::dense(X), n_feat, n_samp, HCLUST_ARGS);
}

int icikt_hclust_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                     int method, double min_raw, int32_t* ma, int32_t* mb, int32_t* msize, double* mraw, double* mcor,
                     int64_t* n_merges, int32_t* component, int64_t* n_components, double* max_taumax,
                     int64_t* reason_counts) {
  return hclust_src(c, MatrixSrc::csc(X), n_feat, n_samp, HCLUST_ARGS);
}

}  // extern "C"
