// icikt_capi_permanova.cpp -- host side of icikt_permanova_f64 / _in / _csc: PERMANOVA (Anderson 2001; vegan::adonis2,
// skbio's permanova) of the samples' classes under the dissimilarity 1 - raw: the sums of the squared dissimilarities
// per class, of the observed labelling and of every permutation, on the device (icikt_permanova.hip).  The whole combn
// triangle runs through the pair engine in blocks of rows; each block's raw values are kept as sortable keys (8 bytes
// per pair, launch_median_keep) before the next block overwrites them.  After the last block one pass turns the keys
// into the fixed-point values q (icikt_fixed.h) and counts the NA pairs; their count and Q come back in the call's one
// wait before the labellings.  The labellings -- the observed one first, then the caller's permutations -- cross PCIe
// in batches and run through the permutation kernel and the class bins, each batch's kernels behind its copy on the
// context's stream.
//
// The rule (icikt_permanova.hip states the device's half; DESIGN.md section 25 the whole): with a single NA pair no
// labelling is summed -- the 1 / n_c weights of the statistic have no meaning on an incomplete class -- and every bin
// is 0; the labels are checked all the same.  This file returns integers only: the statistic needs the bins divided
// by the class sizes of each labelling, and comparing two such sums exactly does not fit 128 bits for arbitrary
// sizes, so F, R2 and n_ge are the front end's (api.permanova_statistic), in fractions.
//
// Device memory: the prepared matrix, one block's buffers (icikt_blocks.h: kTriangleBlockPairs), and
//   16 S (S - 1) / 2                               the kept keys in pair order and their q (S = 65 535: 34 GB): `kept`
//                                                  and `plane_a` of the workspace (icikt_ctx::sel)
//   + 18 S ceil(batch / 16) 16                     a batch of labellings as halfwords and the two limbs of its columns'
//                                                  sums
//   + 16 n_class batch                             the two limbs of the batch's bins
// each with the buffers' growth margin of a ninth.  A batch is sized so that the largest of the three -- labels, column
// sums, bins -- stays within ANO_BATCH_BYTES (64 MB) unless the anoperms plan key says otherwise.  Host memory: one
// batch of labels and 16 bytes per cell of (1 + n_perm) n_class, which is why that product is capped
// (ICIKT_PERMANOVA_MAX_CELLS); the caller's perm_cls is read once, where it lies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
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

struct PermanovaArgs {
  icikt::host::SelectArgs shared;
  const int32_t* cls;
  int n_class;
  const int32_t* perm_cls;
  int64_t n_perm;
  int64_t *n_pairs, *q_total, *bins_lo, *bins_hi;
};

static_assert(ICIKT_PERMANOVA_MAX_CELLS == (1ll << 26), "the header's limit is checked here");

// the body of the three entries: the shared checks, the blocks and the call sequence are select_run's (icikt_host.h)
int permanova_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const PermanovaArgs& A) {
  icikt::host::SelectCall call{c, "permanova", X, n_feat, n_samp, A.shared, {}};
  int rc = icikt::host::select_check_shape(call, "the pairs of the triangle are indexed in 32 bits, a label is a halfword");
  if (rc) return rc;
  rc = icikt::host::select_check_labellings(call, A.cls, A.n_class, ICIKT_ANOSIM_MAX_CLASSES, "a label travels as a halfword",
                                            A.perm_cls, A.n_perm, ICIKT_PERMANOVA_MAX_CELLS);
  if (rc) return rc;
  const int C = A.cls ? A.n_class : 1;   // a null cls: one class, n_class ignored
  if (!A.n_pairs) return fail(c, ICIKT_E_INVALID, "permanova: null output (n_pairs)");
  if (!A.q_total) return fail(c, ICIKT_E_INVALID, "permanova: null output (q_total)");
  if (!A.bins_lo) return fail(c, ICIKT_E_INVALID, "permanova: null output (bins_lo)");
  if (!A.bins_hi) return fail(c, ICIKT_E_INVALID, "permanova: null output (bins_hi)");
  rc = icikt::host::select_check_args(call);
  if (rc) return rc;

  const int64_t S = n_samp;
  const int64_t P = S > 1 ? S * (S - 1) / 2 : 0;
  const int64_t n_lab = 1 + A.n_perm;     // the observed labelling, then the permutations
  unsigned long long h_tot[icikt::PMV_TOTALS] = {0ull, 0ull, 0ull};
  std::vector<unsigned long long> blo, bhi;   // [n_lab][C].  The outputs are written once nothing can fail any more
  try {
    blo.assign((size_t)n_lab * (size_t)C, 0ull);
    bhi.assign((size_t)n_lab * (size_t)C, 0ull);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "permanova: host allocation failed");
  }
  auto write_outputs = [&]() {
    A.n_pairs[0] = P - (int64_t)h_tot[icikt::PMV_T_NA];
    A.n_pairs[1] = (int64_t)h_tot[icikt::PMV_T_NA];
    A.q_total[0] = (int64_t)h_tot[icikt::PMV_T_LO];
    A.q_total[1] = (int64_t)h_tot[icikt::PMV_T_HI];
    for (size_t k = 0; k < blo.size(); ++k) { A.bins_lo[k] = (int64_t)blo[k]; A.bins_hi[k] = (int64_t)bhi[k]; }
  };
  if (n_samp == 0) {   // no column, no pair, no label to check
    write_outputs();
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;

  PairBlocks blocks = PairBlocks::rows(S, budget);
  const int strip = c->plan_ov.anostrip > 0 ? c->plan_ov.anostrip : icikt::ANO_STRIP_DEFAULT;
  // a labelling costs an upload the largest of its labels (2 S bytes), column sums (16 S) and bins (16 C)
  icikt::host::Labellings labs;
  rc = icikt::host::select_labellings_begin(call, A.cls, A.n_class, A.perm_cls, A.n_perm, 16 * std::max<int64_t>(S, C), &labs);
  if (rc) return rc;

  auto& pb = c->pmv;
  auto& ws = c->sel;   // kept, plane_a: the keys, their fixed-point values
  HIPCHK(c, ws.kept.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, ws.plane_a.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, pb.totals.reserve(icikt::PMV_TOTALS));
  HIPCHK(c, pb.colsum_lo.reserve(labs.plan.stage_words));
  HIPCHK(c, pb.colsum_hi.reserve(labs.plan.stage_words));
  HIPCHK(c, pb.bins_lo.reserve((size_t)labs.plan.batch * (size_t)C));
  HIPCHK(c, pb.bins_hi.reserve((size_t)labs.plan.batch * (size_t)C));
  const uint32_t flags = A.shared.flags;

  icikt::host::SelectSteps steps;
  steps.start = [&]() -> int {
    HIPCHK(c, hipMemsetAsync(pb.totals.p, 0, icikt::PMV_TOTALS * sizeof(unsigned long long), c->stream));
    return ICIKT_SUCCESS;
  };
  // a block's raw values as sortable keys, before the next block overwrites them
  steps.fold = [&](const icikt::host::PairBlock& b) -> int { return icikt::host::select_keep_raw(c, b); };
  steps.finish = [&](unsigned long long* red) -> int {
    // the NA pairs say whether anything is left to do: the one wait before the labellings
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, icikt::launch_pmv_quant(ws.kept.p, P, ws.plane_a.p, pb.totals.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(red, c->d_red.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_tot, pb.totals.p, sizeof h_tot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_tot[icikt::PMV_T_NA] > (unsigned long long)P) return fail(c, ICIKT_E_STATE, "permanova: more NA pairs than pairs");
    const bool device = P > 0 && h_tot[icikt::PMV_T_NA] == 0ull;   // an NA pair: nothing is summed, the labels are still checked
    // ---- the labellings (select_labellings): the bins of every one ----
    icikt::host::LabellingSteps per_batch;
    per_batch.launch = [&](int64_t groups, int64_t nb) -> int {
      const size_t words = (size_t)groups * (size_t)S * icikt::ANO_PB;
      HIPCHK(c, hipMemsetAsync(pb.colsum_lo.p, 0, words * sizeof(unsigned long long), c->stream));
      HIPCHK(c, hipMemsetAsync(pb.colsum_hi.p, 0, words * sizeof(unsigned long long), c->stream));
      HIPCHK(c, hipMemsetAsync(pb.bins_lo.p, 0, (size_t)nb * (size_t)C * sizeof(unsigned long long), c->stream));
      HIPCHK(c, hipMemsetAsync(pb.bins_hi.p, 0, (size_t)nb * (size_t)C * sizeof(unsigned long long), c->stream));
      HIPCHK(c, icikt::launch_pmv_perm(ws.plane_a.p, c->labels.p, (int)S, (int)groups, strip, pb.colsum_lo.p, pb.colsum_hi.p,
                                       c->stream));
      HIPCHK(c, icikt::launch_pmv_classes(c->labels.p, pb.colsum_lo.p, pb.colsum_hi.p, (int)S, C, (long long)nb, pb.bins_lo.p,
                                          pb.bins_hi.p, c->stream));
      return ICIKT_SUCCESS;
    };
    per_batch.collect = [&](int64_t q0, int64_t nb) -> int {
      const size_t at = (size_t)q0 * (size_t)C, cells = (size_t)nb * (size_t)C;
      HIPCHK(c, hipMemcpyAsync(blo.data() + at, pb.bins_lo.p, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(bhi.data() + at, pb.bins_hi.p, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      return ICIKT_SUCCESS;
    };
    return icikt::host::select_labellings(call, labs, device, nullptr, per_batch);
  };
  rc = icikt::host::select_run(call, blocks, steps);
  if (!rc) write_outputs();
  return rc;
}

}  // namespace

// (the three entries differ in how the matrix arrives alone)
#define PERMANOVA_ARGS PermanovaArgs{{global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                                     cls, n_class, perm_cls, n_perm, n_pairs, q_total, bins_lo, bins_hi}

extern "C" {

int icikt_permanova_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                        int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                        const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm, int64_t* n_pairs,
                        int64_t* q_total, int64_t* bins_lo, int64_t* bins_hi, double* max_taumax,
                        int64_t* reason_counts) {
  const icikt_input v = icikt::host::f64_view(X, ld);
  return permanova_src(c, MatrixSrc::dense(&v), n_feat, n_samp, PERMANOVA_ARGS);
}

int icikt_permanova_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                       int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                       const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm, int64_t* n_pairs,
                       int64_t* q_total, int64_t* bins_lo, int64_t* bins_hi, double* max_taumax,
                       int64_t* reason_counts) {
  return permanova_src(c, MatrixSrc::dense(X), n_feat, n_samp, PERMANOVA_ARGS);
}

int icikt_permanova_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                        int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                        const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm, int64_t* n_pairs,
                        int64_t* q_total, int64_t* bins_lo, int64_t* bins_hi, double* max_taumax,
                        int64_t* reason_counts) {
  return permanova_src(c, MatrixSrc::csc(X), n_feat, n_samp, PERMANOVA_ARGS);
}

}  // extern "C"
