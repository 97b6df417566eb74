// icikt_capi_mst.cpp -- host side of icikt_mst_f64 / _in / _csc: the maximum spanning forest of the samples under raw,
// which is their single-linkage clustering, found on the device (icikt_mst.hip).  The whole combn triangle runs through
// the pair engine in blocks of rows; each block's raw values are kept as sortable keys (8 bytes per pair,
// launch_median_keep) before the next block overwrites them.  After the last block Boruvka rounds run over the kept
// plane: k_mst_best gives every sample's best edge out of its component, and the host -- O(S) per round -- picks each
// component's best, merges by union-find and uploads the new components.  The tree's S - 1 pairs at most then run
// through the pair engine once more, as a pair list, for their five values.
//
// The rule (icikt_mst.hip states it in full): a pair is a candidate edge iff its raw is not NA and not below min_raw;
// the strict edge order is the larger raw first (colsort::cor_key: -0 equals +0), equal keys by the smaller combn
// index.  The order is total, so the forest is unique, and the edges leave in that order: Kruskal's, the
// single-linkage merge order.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), 8 S (S - 1) / 2 bytes
// of kept keys in the workspace's `kept` plane (icikt_ctx::sel, shared with the other entries; 65 535 samples: 17 GB)
// and 24 S bytes of component labels, live flags and candidates, each with the
// buffers' growth margin of a ninth.  Host memory: O(S), never O(S^2).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::PairBlocks;

namespace {

struct MstArgs {
  icikt::host::SelectArgs shared;
  int scale_max;
  double min_raw;
  int32_t *ti, *tj;
  double* out5t;
  int64_t* n_tree;
  int32_t* component;
  int64_t* n_components;
  int32_t* n_rounds;
};

// an edge of the forest: the key of its raw, its combn index and its ends i < j
struct TreeEdge {
  unsigned long long key;
  int64_t idx;
  int32_t i, j;
};
// the strict edge order
bool edge_before(const TreeEdge& a, const TreeEdge& b) { return a.key != b.key ? a.key > b.key : a.idx < b.idx; }

struct UnionFind {
  std::vector<int32_t> parent, size;
  explicit UnionFind(int64_t n) : parent((size_t)n), size((size_t)n, 1) { std::iota(parent.begin(), parent.end(), 0); }
  int32_t find(int32_t a) {
    while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
    return a;
  }
  bool unite(int32_t a, int32_t b) {
    a = find(a);
    b = find(b);
    if (a == b) return false;
    if (size[a] < size[b]) std::swap(a, b);
    parent[b] = a;
    size[a] += size[b];
    return true;
  }
};

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int mst_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const MstArgs& A) {
  icikt::host::SelectCall call{c, "mst", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits");
  if (rc) return rc;
  if (n_samp > 1 && !A.ti) return fail(c, ICIKT_E_INVALID, "mst: null output (ti)");
  if (n_samp > 1 && !A.tj) return fail(c, ICIKT_E_INVALID, "mst: null output (tj)");
  if (n_samp > 1 && !A.out5t) return fail(c, ICIKT_E_INVALID, "mst: null output (out5t)");
  if (!A.n_tree) return fail(c, ICIKT_E_INVALID, "mst: null output (n_tree)");
  if (n_samp > 0 && !A.component) return fail(c, ICIKT_E_INVALID, "mst: null output (component)");
  if (!A.n_components) return fail(c, ICIKT_E_INVALID, "mst: null output (n_components)");
  if (!A.n_rounds) return fail(c, ICIKT_E_INVALID, "mst: null output (n_rounds)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;
  *A.n_tree = 0;
  *A.n_components = 0;
  *A.n_rounds = 0;
  if (n_samp == 0) return ICIKT_SUCCESS;
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const int64_t S = n_samp;
  const uint32_t flags = A.shared.flags;
  const unsigned long long min_key = A.min_raw == A.min_raw ? icikt::host::cor_key(A.min_raw) : 0ull;   // NaN: no bound
  PairBlocks blocks = PairBlocks::rows(S, budget);
  auto& mb = c->mst;
  HIPCHK(c, c->sel.kept.reserve((size_t)std::max<int64_t>(blocks.total, 1)));
  HIPCHK(c, mb.comp.reserve((size_t)S));
  HIPCHK(c, mb.live.reserve((size_t)S));
  HIPCHK(c, mb.best.reserve((size_t)S));

  // the forest as the rounds record it, then in the strict order; the values of its pairs; the rounds run
  std::vector<TreeEdge> tree;
  std::vector<double> out4;
  std::vector<int32_t> comp, live;
  int rounds = 0;
  int64_t n_comp = 0;
  unsigned long long red0 = 0ull;   // word 0 of launch_out_stats' record: the largest taumax as a key (0: no pair had one)

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int { return ICIKT_SUCCESS; };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    std::vector<icikt::MstBest> best;
    std::vector<unsigned long long> ckey;
    std::vector<TreeEdge> cbest, chosen;
    std::vector<int32_t> pi, pj, reasons;
    try {
      comp.resize((size_t)S);
      std::iota(comp.begin(), comp.end(), 0);
      live.assign((size_t)S, 1);
      best.resize((size_t)S);
      ckey.resize((size_t)S);
      cbest.resize((size_t)S);
      tree.reserve((size_t)(S - 1));
    } catch (const std::bad_alloc&) {
      return fail(c, ICIKT_E_NOMEM, "mst: host allocation failed");
    }
    UnionFind uf(S);
    // ---- Boruvka rounds: bounded, never a loop that waits for a condition ----
    int64_t live_comps = S;
    bool ended = false;
    for (int round = 0; round < icikt::MST_MAX_ROUNDS && !ended; ++round) {
      if (live_comps <= 1) { ended = true; break; }   // one component left that may still have a candidate: it has none
      int r = icikt::host::upload_sync(c, mb.comp.p, comp.data(), (size_t)S * sizeof(int32_t));
      if (!r) r = icikt::host::upload_sync(c, mb.live.p, live.data(), (size_t)S * sizeof(int32_t));
      if (!r) r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
      if (r) return r;
      HIPCHK(c, icikt::launch_mst_best(c->sel.kept.p, mb.comp.p, mb.live.p, min_key, (int)S, mb.best.p, c->stream));
      r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
      if (r) return r;
      HIPCHK(c, hipMemcpyAsync(best.data(), mb.best.p, (size_t)S * sizeof(icikt::MstBest), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      ++rounds;
      // every component's best candidate in the strict order: the full combn index decides among its members
      std::fill(ckey.begin(), ckey.end(), 0ull);
      bool any = false;
      for (int64_t s = 0; s < S; ++s) {
        const icikt::MstBest& b = best[(size_t)s];
        if (!live[(size_t)s] || !b.key) continue;
        if (b.t < 0 || b.t >= S || b.t == s || comp[(size_t)b.t] == comp[(size_t)s] || b.key == icikt::host::NA_KEY)
          return fail(c, ICIKT_E_STATE, "mst: sample " + std::to_string(s) + " came back with a candidate that is no edge out of its component");
        const int32_t i = (int32_t)std::min<int64_t>(s, b.t), j = (int32_t)std::max<int64_t>(s, b.t);
        const TreeEdge e{b.key, icikt::host::row_offset(S, i) + (j - i - 1), i, j};
        const size_t root = (size_t)comp[(size_t)s];
        if (!ckey[root] || edge_before(e, cbest[root])) { ckey[root] = e.key; cbest[root] = e; }
        any = true;
      }
      // a component without a candidate has none in any later round either: its samples are skipped from now on
      for (int64_t s = 0; s < S; ++s)
        if (live[(size_t)s] && !ckey[(size_t)comp[(size_t)s]]) live[(size_t)s] = 0;
      if (!any) { ended = true; break; }
      chosen.clear();
      for (int64_t s = 0; s < S; ++s)
        if (comp[(size_t)s] == s && ckey[(size_t)s]) chosen.push_back(cbest[(size_t)s]);
      // an edge chosen from both sides is recorded once; under a total order the chosen edges close no cycle
      std::sort(chosen.begin(), chosen.end(), [](const TreeEdge& a, const TreeEdge& b) { return a.idx < b.idx; });
      chosen.erase(std::unique(chosen.begin(), chosen.end(), [](const TreeEdge& a, const TreeEdge& b) { return a.idx == b.idx; }),
                   chosen.end());
      int64_t merged = 0;
      for (const TreeEdge& e : chosen) {
        if (!uf.unite(e.i, e.j))
          return fail(c, ICIKT_E_STATE, "mst: a round's chosen edges close a cycle (pair " + std::to_string(e.i) + ", " + std::to_string(e.j) + ")");
        tree.push_back(e);
        ++merged;
      }
      if (merged == 0) return fail(c, ICIKT_E_STATE, "mst: a round merged nothing while candidates exist");
      live_comps = 0;
      for (int64_t s = 0; s < S; ++s) {
        comp[(size_t)s] = uf.find((int32_t)s);
        if (comp[(size_t)s] == s && live[(size_t)s]) ++live_comps;   // (a root carries its component's flag: the flags of a
      }                                                               //  component's samples are equal, merged ones were all live)
    }
    if (!ended && live_comps > 1)
      return fail(c, ICIKT_E_STATE, "mst: the rounds did not end within " + std::to_string(icikt::MST_MAX_ROUNDS));
    // ---- components, numbered in order of their smallest sample; the invariant ----
    n_comp = 0;
    std::fill(live.begin(), live.end(), -1);   // (the flags are through: from here on the roots' numbers)
    for (int64_t s = 0; s < S; ++s) {
      const size_t root = (size_t)uf.find((int32_t)s);
      if (live[root] < 0) live[root] = (int32_t)n_comp++;
      comp[(size_t)s] = (int32_t)root;
    }
    for (int64_t s = 0; s < S; ++s) comp[(size_t)s] = live[(size_t)comp[(size_t)s]];
    const int64_t n_tree = (int64_t)tree.size();
    if (n_tree + n_comp != S)
      return fail(c, ICIKT_E_STATE, "mst: " + std::to_string(n_tree) + " edges and " + std::to_string(n_comp) +
                                        " components do not add up to " + std::to_string(S) + " samples");
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    red0 = red[0];
    if (n_tree == 0) return ICIKT_SUCCESS;
    // ---- the five values of the tree's pairs: the pair engine over the tree as a pair list, in the strict order.  No
    // second launch_out_stats_accum: d_red has counted every pair of the triangle once ----
    std::sort(tree.begin(), tree.end(), edge_before);
    try {
      pi.resize((size_t)n_tree);
      pj.resize((size_t)n_tree);
      out4.resize(4 * (size_t)n_tree);
      reasons.resize((size_t)n_tree);
    } catch (const std::bad_alloc&) {
      return fail(c, ICIKT_E_NOMEM, "mst: host allocation failed");
    }
    for (int64_t e = 0; e < n_tree; ++e) { pi[(size_t)e] = tree[(size_t)e].i; pj[(size_t)e] = tree[(size_t)e].j; }
    int r = icikt_set_pairs(c, pi.data(), pj.data(), n_tree);
    if (!r) r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    const uint32_t quiet = flags & ~(uint32_t)(ICIKT_FLAG_REUSE_COUNTS | ICIKT_FLAG_TIMING);   // one timer pair around both kernels
    r = icikt_run_dev(c, A.shared.perspective, A.shared.alternative, A.shared.continuity, quiet, c->d_out4.p, nullptr,
                      c->d_reasons.p);
    if (!r) r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(out4.data(), c->d_out4.p, 4 * (size_t)n_tree * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(reasons.data(), c->d_reasons.p, (size_t)n_tree * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t e = 0; e < n_tree; ++e) {
      const double raw = out4[4 * (size_t)e];
      if (reasons[(size_t)e] != 0 || icikt::host::cor_key(raw) != tree[(size_t)e].key)
        return fail(c, ICIKT_E_STATE, "mst: the pair (" + std::to_string(pi[(size_t)e]) + ", " + std::to_string(pj[(size_t)e]) +
                                          ") of the tree has another raw as a pair list than in the triangle");
    }
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (rc) return rc;

  // the outputs, once nothing can fail any more; the slots behind n_tree stay untouched
  const int64_t n_tree = (int64_t)tree.size();
  const double max_cor = icikt::host::max_taumax_of(red0);
  const size_t plane = (size_t)(S - 1);
  for (int64_t e = 0; e < n_tree; ++e) {
    const double raw = out4[4 * (size_t)e];
    A.ti[e] = tree[(size_t)e].i;
    A.tj[e] = tree[(size_t)e].j;
    A.out5t[(size_t)e] = A.scale_max ? raw / max_cor : raw;   // k_assemble's expression on k_assemble's operands
    A.out5t[plane + (size_t)e] = raw;
    A.out5t[2 * plane + (size_t)e] = out4[4 * (size_t)e + 1];
    A.out5t[3 * plane + (size_t)e] = out4[4 * (size_t)e + 2];
    A.out5t[4 * plane + (size_t)e] = out4[4 * (size_t)e + 3];
  }
  for (int64_t s = 0; s < S; ++s) A.component[s] = comp[(size_t)s];
  *A.n_tree = n_tree;
  *A.n_components = n_comp;
  *A.n_rounds = rounds;
  return ICIKT_SUCCESS;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define MST_ARGS MstArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                         scale_max, min_raw, ti, tj, out5t, n_tree, component, n_components, n_rounds}

extern "C" {

int icikt_mst_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                  int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  double min_raw, int32_t* ti, int32_t* tj, double* out5t, int64_t* n_tree, int32_t* component,
                  int64_t* n_components, int32_t* n_rounds, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return mst_src(c, MatrixSrc::dense(&v), n_feat, n_samp, MST_ARGS);
}

int icikt_mst_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                 int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                 double min_raw, int32_t* ti, int32_t* tj, double* out5t, int64_t* n_tree, int32_t* component,
                 int64_t* n_components, int32_t* n_rounds, double* max_taumax, int64_t* reason_counts) {
  return mst_src(c, MatrixSrc::dense(X), n_feat, n_samp, MST_ARGS);
}

int icikt_mst_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                  int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  double min_raw, int32_t* ti, int32_t* tj, double* out5t, int64_t* n_tree, int32_t* component,
                  int64_t* n_components, int32_t* n_rounds, double* max_taumax, int64_t* reason_counts) {
  return mst_src(c, MatrixSrc::csc(X), n_feat, n_samp, MST_ARGS);
}

}  // extern "C"
