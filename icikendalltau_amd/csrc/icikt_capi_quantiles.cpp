// icikt_capi_quantiles.cpp -- host side of icikt_quantiles_f64 / _in / _csc: exact quantiles (R's type 7) and a
// histogram of raw over all C(S, 2) pairs, split into all / within-class / between-class pairs, reduced on the device
// (icikt_quantiles.hip).  The combn triangle runs through the pair engine in blocks of whole rows; each block is folded
// into the histogram and the counts, and -- when quantiles are asked for -- its raw values are kept as sortable keys
// (8 bytes per pair).  After the last block the counts come back in the call's one wait, the host turns them into the
// ranks of the order statistics, and a radix select over the kept plane finds their keys.  The device delivers order
// statistics and the scale m only: the interpolation runs here, in plain C++ with no fused multiply-add.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   (n_probs > 0 ? 8 S (S - 1) / 2 : 0)            the kept keys, in the workspace's `kept` plane (icikt_ctx::sel,
//                                                  shared with the other entries; S = 65 535: 17 GB); group membership
//                                                  is recomputed from a pair's index: no ninth byte per pair
//   + 4 S                                          the class index (with cls)
//   + 8 n_breaks + 16 (4 + n_breaks - 1)           the breaks, the totals of the two counted groups
//   + 20 * 192 + 8 * 32 * 256                      the select's targets and one batch's digit histograms
// each with the buffers' growth margin of a ninth.  Host memory: O(S + n_breaks + n_probs), never O(pairs).
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

struct QuantArgs {
  icikt::host::SelectArgs shared;
  const int32_t* cls;
  int n_class, scale_max;
  const double* probs;
  int n_probs;
  const double* breaks;
  int n_breaks;
  double *q2, *order2;
  int64_t *n_valid, *n_na, *hist, *outside;
};

// what the device delivers: per group the counts, and per (group, prob, lo | hi) an order statistic as its key
struct QuantFound {
  int64_t n_valid[3] = {}, n_na[3] = {}, below[3] = {}, above[3] = {};
  std::vector<int64_t> hist;                  // [n_group][n_bins]
  std::vector<int> target;                    // [n_group][n_probs][2]: index into key, -1 without a value
  std::vector<unsigned long long> key;        // per distinct (group, rank)
  std::vector<double> index, lo;              // [n_group][n_probs]: 1 + (v - 1) p and its floor
};

double plus_zero(double v) { return v == 0.0 ? 0.0 : v; }

// R's quantile(type = 7) between the order statistics a = x[lo] and b = x[hi], index = 1 + (v - 1) p.  Every product
// and sum is rounded on its own: no contraction into a fused multiply-add, whatever the target's flags.
double type7_index(int64_t v, double p) {
#pragma clang fp contract(off)
  const double scaled = (double)(v - 1) * p;
  return 1.0 + scaled;
}
double type7_value(double a, double b, double index, double lo) {
#pragma clang fp contract(off)
  if (index == lo || a == b) return plus_zero(a);
  const double h = index - lo;
  const double wa = (1.0 - h) * a, wb = h * b;
  return plus_zero(wa + wb);
}

// the distinct (group, rank) of the call: found.target, found.index / lo; ranks and groups of the targets
void plan_targets(const QuantArgs& A, int n_group, QuantFound* f, std::vector<long long>* rank, std::vector<int32_t>* group) {
  const int np = A.n_probs;
  f->target.assign((size_t)n_group * np * 2, -1);
  f->index.assign((size_t)n_group * np, 0.0);
  f->lo.assign((size_t)n_group * np, 0.0);
  for (int g = 0; g < n_group; ++g) {
    const int64_t v = f->n_valid[g];
    if (v == 0) continue;
    for (int p = 0; p < np; ++p) {
      const double index = type7_index(v, A.probs[p]);
      const double lo = std::floor(index), hi = std::ceil(index);
      f->index[(size_t)g * np + p] = index;
      f->lo[(size_t)g * np + p] = lo;
      const long long want[2] = {std::min<long long>(std::max<long long>((long long)lo, 1), v) - 1,
                                 std::min<long long>(std::max<long long>((long long)hi, 1), v) - 1};
      for (int q = 0; q < 2; ++q) {
        size_t t = 0;
        while (t < rank->size() && !((*group)[t] == g && (*rank)[t] == want[q])) ++t;
        if (t == rank->size()) {
          rank->push_back(want[q]);
          group->push_back(g);
        }
        f->target[((size_t)g * np + p) * 2 + q] = (int)t;
      }
    }
  }
  f->key.assign(rank->size(), 0ull);
}

// the caller's arrays from what was found; m: cor's denominator
void write_outputs(const QuantArgs& A, int n_group, const QuantFound& f, double m) {
  const int np = A.n_probs, n_bins = A.n_breaks > 0 ? A.n_breaks - 1 : 0;
  for (int g = 0; g < n_group; ++g) {
    if (A.n_valid) A.n_valid[g] = f.n_valid[g];
    if (A.n_na) A.n_na[g] = f.n_na[g];
    if (A.outside) {
      A.outside[2 * g] = f.below[g];
      A.outside[2 * g + 1] = f.above[g];
    }
    for (int k = 0; k < n_bins; ++k) A.hist[(size_t)g * n_bins + k] = f.hist[(size_t)g * n_bins + k];
    for (int p = 0; p < np; ++p) {
      const size_t cell = (size_t)g * np + p;
      double a = icikt::host::from_bits(icikt::host::R_NA_BITS), b = a, qr = a, qc = a;
      if (f.target[cell * 2] >= 0) {
        a = icikt::host::cor_key_value(f.key[(size_t)f.target[cell * 2]]);
        b = icikt::host::cor_key_value(f.key[(size_t)f.target[cell * 2 + 1]]);
        qr = type7_value(a, b, f.index[cell], f.lo[cell]);
        // the division is k_assemble's, on k_assemble's operands; max(numeric(0), na.rm = TRUE) is -Inf in R
        qc = A.scale_max ? type7_value(plus_zero(a / m), plus_zero(b / m), f.index[cell], f.lo[cell]) : qr;
      }
      A.order2[cell * 2] = a;
      A.order2[cell * 2 + 1] = b;
      A.q2[cell] = qc;
      A.q2[(size_t)n_group * np + cell] = qr;
    }
  }
}

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int quantiles_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const QuantArgs& A) {
  icikt::host::SelectCall call{c, "quantiles", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "a pair's columns are recomputed from its index in the triangle");
  if (rc) return rc;
  rc = icikt::host::select_check_classes(call, A.cls, A.n_class);
  if (rc) return rc;
  if (A.n_probs < 0 || A.n_probs > ICIKT_QUANTILE_MAX_PROBS)
    return fail(c, ICIKT_E_INVALID, "quantiles: n_probs must be in 0 .. ICIKT_QUANTILE_MAX_PROBS (32)");
  if (A.n_probs > 0 && !A.probs) return fail(c, ICIKT_E_INVALID, "quantiles: null probs");
  for (int p = 0; p < A.n_probs; ++p)
    if (!(A.probs[p] >= 0.0 && A.probs[p] <= 1.0))
      return fail(c, ICIKT_E_INVALID, "quantiles: probs[" + std::to_string(p) + "] = " + std::to_string(A.probs[p]) +
                                          " is outside [0, 1]");
  if (A.n_breaks != 0 && (A.n_breaks < 2 || A.n_breaks > ICIKT_HIST_MAX_BINS + 1))
    return fail(c, ICIKT_E_INVALID, "quantiles: n_breaks must be 0 or in 2 .. ICIKT_HIST_MAX_BINS + 1 (1025)");
  if (A.n_breaks > 0 && !A.breaks) return fail(c, ICIKT_E_INVALID, "quantiles: null breaks");
  for (int k = 0; k < A.n_breaks; ++k) {
    if (!std::isfinite(A.breaks[k]))
      return fail(c, ICIKT_E_INVALID, "quantiles: breaks[" + std::to_string(k) + "] = " + std::to_string(A.breaks[k]) + " is not finite");
    if (k > 0 && !(A.breaks[k] > A.breaks[k - 1]))
      return fail(c, ICIKT_E_INVALID, "quantiles: breaks[" + std::to_string(k) + "] = " + std::to_string(A.breaks[k]) +
                                          " is not above breaks[" + std::to_string(k - 1) + "]");
  }
  if (A.n_probs > 0 && !A.q2) return fail(c, ICIKT_E_INVALID, "quantiles: null output (q2)");
  if (A.n_probs > 0 && !A.order2) return fail(c, ICIKT_E_INVALID, "quantiles: null output (order2)");
  if (A.n_breaks > 0 && !A.hist) return fail(c, ICIKT_E_INVALID, "quantiles: null output (hist)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int n_group = A.cls ? 3 : 1, n_counted = A.cls ? 2 : 1;
  const int n_bins = A.n_breaks > 0 ? A.n_breaks - 1 : 0;
  const int stride = icikt::QUANT_HEAD + n_bins;   // words of a counted group's totals
  QuantFound found;
  std::vector<long long> t_rank;
  std::vector<int32_t> t_group;
  std::vector<unsigned long long> h_tot;
  try {
    found.hist.assign((size_t)n_group * n_bins, 0);
    h_tot.assign((size_t)n_counted * stride, 0ull);
    t_rank.reserve(2 * 3 * ICIKT_QUANTILE_MAX_PROBS);
    t_group.reserve(2 * 3 * ICIKT_QUANTILE_MAX_PROBS);
    if (n_samp == 0) {   // no column, no pair: every count 0, every quantile NA
      plan_targets(A, n_group, &found, &t_rank, &t_group);
      write_outputs(A, n_group, found, 1.0);
      return ICIKT_SUCCESS;
    }
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "quantiles: host allocation failed");
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  const int64_t S = n_samp;
  PairBlocks blocks = PairBlocks::rows(S, budget);
  const int64_t P = blocks.total;
  const int batch = c->plan_ov.qbatch > 0 ? c->plan_ov.qbatch : icikt::QUANT_BATCH_MAX;
  const size_t max_targets = 2 * 3 * (size_t)ICIKT_QUANTILE_MAX_PROBS;
  auto& qb = c->quant;
  if (A.n_probs > 0) HIPCHK(c, c->sel.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, qb.totals.reserve((size_t)n_counted * stride));
  HIPCHK(c, qb.prefix.reserve(max_targets));
  HIPCHK(c, qb.rank.reserve(max_targets));
  HIPCHK(c, qb.group.reserve(max_targets));
  HIPCHK(c, qb.hist.reserve((size_t)icikt::QUANT_BATCH_MAX * 256));
  if (A.cls) HIPCHK(c, qb.cls.reserve((size_t)S));
  if (A.n_breaks > 0) HIPCHK(c, qb.breaks.reserve((size_t)A.n_breaks));
  const int32_t* const d_cls = A.cls ? qb.cls.p : nullptr;
  unsigned long long* const d_kept = A.n_probs > 0 ? c->sel.kept.p : nullptr;
  const uint32_t flags = A.shared.flags;
  double m = 1.0;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    int r = ICIKT_SUCCESS;
    if (A.cls) r = icikt::host::upload_sync(c, qb.cls.p, A.cls, (size_t)S * sizeof(int32_t));
    if (!r && A.n_breaks > 0) r = icikt::host::upload_sync(c, qb.breaks.p, A.breaks, (size_t)A.n_breaks * sizeof(double));
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(qb.totals.p, 0, (size_t)n_counted * stride * sizeof(unsigned long long), c->stream));
    return ICIKT_SUCCESS;
  };
  // a block's histogram and counts, and its raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int {
    HIPCHK(c, icikt::launch_quant_fold(c->d_out4.p, c->d_reasons.p, b.count, b.begin, (int)S, d_cls, qb.breaks.p,
                                       A.n_breaks, d_kept, qb.totals.p, c->stream));
    return ICIKT_SUCCESS;
  };
  steps.finish = [&](unsigned long long* red) -> int {
    // n_valid decides the ranks to look for: the one wait inside the call
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_tot.data(), qb.totals.p, h_tot.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // group 2 is what group 0 holds and group 1 does not: every pair is in exactly one of 1 and 2
    auto word = [&](int g, int w) -> int64_t {
      const int64_t all = (int64_t)h_tot[(size_t)w], in = n_counted > 1 ? (int64_t)h_tot[(size_t)stride + w] : 0;
      return g == 0 ? all : (g == 1 ? in : all - in);
    };
    for (int g = 0; g < n_group; ++g) {
      found.n_valid[g] = word(g, 0);
      found.n_na[g] = word(g, 1);
      found.below[g] = word(g, 2);
      found.above[g] = word(g, 3);
      for (int k = 0; k < n_bins; ++k) found.hist[(size_t)g * n_bins + k] = word(g, icikt::QUANT_HEAD + k);
    }
    if (A.scale_max) m = icikt::host::max_taumax_of(red[0]);
    try { plan_targets(A, n_group, &found, &t_rank, &t_group); } catch (const std::bad_alloc&) {
      return fail(c, ICIKT_E_NOMEM, "quantiles: host allocation failed");
    }
    const int n_t = (int)t_rank.size();
    if (n_t == 0) return ICIKT_SUCCESS;
    if ((size_t)n_t > max_targets) return fail(c, ICIKT_E_STATE, "quantiles: more targets than the call can have");
    int r = icikt::host::upload_sync(c, qb.rank.p, t_rank.data(), (size_t)n_t * sizeof(long long));
    if (!r) r = icikt::host::upload_sync(c, qb.group.p, t_group.data(), (size_t)n_t * sizeof(int32_t));
    if (r) return r;
    const icikt::QuantTargets T{qb.prefix.p, qb.rank.p, qb.group.p};
    r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(qb.prefix.p, 0, (size_t)n_t * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(qb.hist.p, 0, (size_t)icikt::QUANT_BATCH_MAX * 256 * sizeof(unsigned long long), c->stream));
    for (int t0 = 0; t0 < n_t; t0 += batch) {
      const int nt = std::min(batch, n_t - t0);
      for (int shift = 56; shift >= 0; shift -= 8) {
        HIPCHK(c, icikt::launch_quant_count(d_kept, P, (int)S, d_cls, T, t0, nt, shift, qb.hist.p, c->stream));
        HIPCHK(c, icikt::launch_quant_pick(T, t0, nt, shift, qb.hist.p, c->stream));
      }
    }
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(found.key.data(), qb.prefix.p, (size_t)n_t * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICIKT_SUCCESS;
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) write_outputs(A, n_group, found, m);
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define QUANT_ARGS QuantArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                             cls, n_class, scale_max, probs, n_probs, breaks, n_breaks, q2, order2, n_valid, n_na, hist, outside}

extern "C" {

int icikt_quantiles_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                        const double* global_na, int n_global_na, const int32_t* cls, int n_class, int perspective,
                        int alternative, int continuity, uint32_t flags, int scale_max, const double* probs, int n_probs,
                        const double* breaks, int n_breaks, double* q2, double* order2, int64_t* n_valid, int64_t* n_na,
                        int64_t* hist, int64_t* outside, double* max_taumax, int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return quantiles_src(c, MatrixSrc::dense(&v), n_feat, n_samp, QUANT_ARGS);
}

int icikt_quantiles_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                       int n_global_na, const int32_t* cls, int n_class, int perspective, int alternative,
                       int continuity, uint32_t flags, int scale_max, const double* probs, int n_probs,
                       const double* breaks, int n_breaks, double* q2, double* order2, int64_t* n_valid, int64_t* n_na,
                       int64_t* hist, int64_t* outside, double* max_taumax, int64_t* reason_counts) {
  return quantiles_src(c, MatrixSrc::dense(X), n_feat, n_samp, QUANT_ARGS);
}

int icikt_quantiles_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                        int n_global_na, const int32_t* cls, int n_class, int perspective, int alternative,
                        int continuity, uint32_t flags, int scale_max, const double* probs, int n_probs,
                        const double* breaks, int n_breaks, double* q2, double* order2, int64_t* n_valid, int64_t* n_na,
                        int64_t* hist, int64_t* outside, double* max_taumax, int64_t* reason_counts) {
  return quantiles_src(c, MatrixSrc::csc(X), n_feat, n_samp, QUANT_ARGS);
}

}  // extern "C"
