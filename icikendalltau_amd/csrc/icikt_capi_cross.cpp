// icikt_capi_cross.cpp -- host side of the query x reference rectangle: the ICI-Kendall-tau of every column of a query
// matrix with every column of a reference matrix, as five Sq x Sr matrices and / or as every query's k best reference
// columns and / or as every query's median to every class of a labelled reference (icikt_cross.hip).
//   icikt_cross_f64 / _in      both matrices arrive with the call.  The device matrix holds the query columns, one
//                              all-missing padding column when Sq is odd (the reference must start on an even column: the
//                              pre-pass's tables are interleaved in blocks of two), then the reference columns.
//   icikt_ref_prepare_f64 / _in, icikt_ref_cross_f64 / _in, icikt_ref_info
//                              the reference is uploaded and pre-passed ONCE and stays on the context; a batch brings its
//                              query columns alone.  The mirror layout: the reference in device columns 0 .. Sr - 1, one
//                              padding column when Sr is odd, the batch from ref_query_col(Sr) on.
// Either way the rectangle runs through the selection entries' driver (select_run) in blocks of whole query rows
// (PairBlocks::rect / rect_ref_first), and each block is folded before the next one overwrites its records: cross_run
// below is the one body of both.
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

struct CrossArgs {
  icikt::host::SelectArgs shared;
  int k, scale_max;
  double* out5;
  int32_t* idx;
  double* out5k;
  int32_t* n_valid;
  // a labelled reference (icikt_ref_cross_* alone; null / 0 in icikt_cross_*)
  const int32_t* ref_cls;
  int n_class;
  double* cls_med2;
  int32_t* cls_n_valid;
};

inline bool want_topk(const CrossArgs& A) { return A.idx || A.out5k || A.n_valid; }
inline bool want_class(const CrossArgs& A) { return A.cls_med2 || A.cls_n_valid; }

// the checks both entries make of their outputs, k and the classes, `who` prefixing the message
int cross_check_outputs(icikt_ctx* c, const std::string& who, const CrossArgs& A, int64_t Sr) {
  if (!A.out5 && !want_topk(A) && !want_class(A) && !A.shared.max_taumax && !A.shared.reason_counts)
    return fail(c, ICIKT_E_INVALID, who + ": all outputs are null");
  if (want_topk(A) && (A.k < 1 || A.k > ICIKT_TOPK_MAX))
    return fail(c, ICIKT_E_INVALID, who + ": k must be in 1 .. ICIKT_TOPK_MAX (256)");
  if (want_class(A) && !A.ref_cls) return fail(c, ICIKT_E_INVALID, who + ": a class table needs ref_cls");
  if (A.ref_cls) {
    if (A.n_class < 1 || A.n_class > icikt::CLASS_MATRIX_MAX_CLASSES)
      return fail(c, ICIKT_E_INVALID, who + ": n_class must be in 1 .. 65535 (the classes are the second dimension of the "
                                            "class kernel's grid)");
    return icikt::host::check_labels(c, who.c_str(), "ref_cls", A.ref_cls, Sr, A.n_class);
  }
  return ICIKT_SUCCESS;
}

// no pair: the matrices are empty, every list is padding, every class cell is without a partner
void cross_empty(const CrossArgs& A, int64_t Sq) {
  const size_t SK = (size_t)Sq * (want_topk(A) ? (size_t)A.k : 0), SC = (size_t)Sq * (size_t)(A.ref_cls ? A.n_class : 0);
  const double NA = icikt::host::from_bits(icikt::host::R_NA_BITS);
  for (size_t t = 0; A.idx && t < SK; ++t) A.idx[t] = -1;
  for (size_t t = 0; A.out5k && t < 5 * SK; ++t) A.out5k[t] = NA;
  for (int64_t q = 0; A.n_valid && q < Sq; ++q) A.n_valid[q] = 0;
  for (size_t t = 0; A.cls_med2 && t < 2 * SC; ++t) A.cls_med2[t] = NA;
  for (size_t t = 0; A.cls_n_valid && t < SC; ++t) A.cls_n_valid[t] = 0;
}

// The one body: the Sq x Sr rectangle (both at least 1) in `blocks`, the device matrix brought by `upload`, the folds,
// the cor step and the downloads.  The checks are the caller's; leaves the context as select_run does.
int cross_run(icikt::host::SelectCall& call, int64_t Sq, int64_t Sr, const CrossArgs& A, PairBlocks& blocks,
              const std::function<int()>& upload) {
  icikt_ctx* const c = call.c;
  const bool topk = want_topk(A), classes = want_class(A);
  const size_t k = topk ? (size_t)A.k : 0, SK = (size_t)Sq * k, P = (size_t)Sq * (size_t)Sr;
  const int C = classes ? A.n_class : 0;
  const size_t SC = (size_t)Sq * (size_t)C;
  auto& cx = c->cross;
  // the reference columns sorted stably by class (class_index) and each class's range in that list
  std::vector<int32_t> member, first;
  if (classes) {
    try {
      member = icikt::host::class_index(A.ref_cls, Sr).runs.member;
      first.assign((size_t)C + 1, 0);
      for (int64_t r = 0; r < Sr; ++r) ++first[(size_t)A.ref_cls[r] + 1];
      for (int q = 0; q < C; ++q) first[(size_t)q + 1] += first[(size_t)q];
    } catch (const std::bad_alloc&) {
      return fail(c, ICIKT_E_NOMEM, std::string(call.who) + ": host allocation failed");
    }
    HIPCHK(c, cx.member.reserve((size_t)Sr));
    HIPCHK(c, cx.first.reserve((size_t)C + 1));
    HIPCHK(c, cx.med2.reserve(2 * SC));
    HIPCHK(c, cx.cls_n_valid.reserve(SC));
  }
  if (A.out5) HIPCHK(c, cx.planes.reserve(5 * P));
  if (topk) {
    HIPCHK(c, cx.idx.reserve(SK));
    HIPCHK(c, cx.out.reserve(5 * SK));
    HIPCHK(c, cx.n_valid.reserve((size_t)Sq));
  }
  const uint32_t flags = A.shared.flags;
  const int stage = c->plan_ov.medlds >= 0 ? c->plan_ov.medlds : icikt::MEDIAN_STAGE_MAX;

  icikt::host::SelectSteps steps;
  steps.upload = upload;
  steps.start = [&]() -> int {
    if (!classes) return ICIKT_SUCCESS;
    int r = icikt::host::upload_sync(c, cx.member.p, member.data(), (size_t)Sr * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, cx.first.p, first.data(), ((size_t)C + 1) * sizeof(int32_t));
    return r;
  };
  steps.fold = [&](const icikt::host::PairBlock& b) -> int {
    const int rows = b.row_last - b.row_first;
    if (topk)
      HIPCHK(c, icikt::launch_cross_topk(c->d_out4.p, (int)Sr, (int)k, b.row_first, rows, (long long)Sq, cx.idx.p, cx.out.p,
                                         cx.n_valid.p, c->stream));
    if (classes)
      HIPCHK(c, icikt::launch_cross_class(c->d_out4.p, cx.member.p, cx.first.p, (int)Sr, C, b.row_first, rows, (long long)Sq,
                                          stage, cx.med2.p, cx.cls_n_valid.p, c->stream));
    if (A.out5) HIPCHK(c, icikt::launch_cross_planes(c->d_out4.p, b.count, b.begin, (long long)P, cx.planes.p, c->stream));
    return ICIKT_SUCCESS;
  };
  steps.finish = [&](unsigned long long* red) -> int {
    int r = icikt::host::timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    const int scale = A.scale_max ? 1 : 0;
    if (topk) HIPCHK(c, icikt::launch_cross_cor(c->d_red.p, scale, cx.idx.p, (long long)SK, cx.out.p, c->stream));
    if (classes) HIPCHK(c, icikt::launch_cross_class_cor(c->d_red.p, scale, cx.cls_n_valid.p, (long long)SC, cx.med2.p, c->stream));
    if (A.out5) HIPCHK(c, icikt::launch_cross_cor(c->d_red.p, scale, nullptr, (long long)P, cx.planes.p, c->stream));
    r = icikt::host::timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (!r && A.idx) r = icikt::host::download(c, A.idx, cx.idx.p, SK * sizeof(int32_t));
    if (!r && A.out5k) r = icikt::host::download(c, A.out5k, cx.out.p, 5 * SK * sizeof(double));
    if (!r && A.n_valid) r = icikt::host::download(c, A.n_valid, cx.n_valid.p, (size_t)Sq * sizeof(int32_t));
    if (!r && A.cls_med2) r = icikt::host::download(c, A.cls_med2, cx.med2.p, 2 * SC * sizeof(double));
    if (!r && A.cls_n_valid) r = icikt::host::download(c, A.cls_n_valid, cx.cls_n_valid.p, SC * sizeof(int32_t));
    if (!r && A.out5) r = icikt::host::download(c, A.out5, cx.planes.p, 5 * P * sizeof(double));
    if (!r) r = icikt::host::select_download_red(c, red);
    return r;
  };
  return icikt::host::select_run(call, blocks, steps);
}

// the padding column `col` of the device matrix: all missing, pre-passed like any column, in no pair
int pad_column(icikt_ctx* c, int64_t n_feat, int64_t col, uint32_t flags) {
  int r = icikt::host::timer_begin(c, ICIKT_K_PREPARE, flags);
  if (r) return r;
  HIPCHK(c, icikt::launch_cross_pad(c->d_X.p + (size_t)col * (size_t)n_feat, (int)n_feat, c->stream));
  r = icikt::host::prepare_launch(c, c->d_X.p, n_feat, col, col + 1);
  if (!r) r = icikt::host::timer_end(c, ICIKT_K_PREPARE, flags);
  return r;
}

// icikt_cross_*: Q is n_feat x Sq, R is n_feat x Sr
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
  rc = cross_check_outputs(c, "cross", A, Sr);
  if (!rc) rc = icikt::host::select_check_args(call);
  if (rc) return rc;
  if (Sq == 0 || Sr == 0) {
    cross_empty(A, Sq);
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;
  PairBlocks blocks = PairBlocks::rect(Sq, Sr, budget);
  const uint32_t flags = A.shared.flags;
  const std::function<int()> upload = [&]() -> int {
    // d_X for all columns BEFORE the first upload: a DevBuf that grows drops what it holds
    HIPCHK(c, c->d_X.reserve((size_t)std::max<int64_t>(n_feat * S_dev, 1)));
    int r = icikt::host::prepare_alloc(c, n_feat, S_dev, S_dev, S_dev);
    if (r) return r;
    c->k0_mask = &call.ms;
    c->k0_keep = nullptr;
    r = icikt::host::upload_and_prepare(c, Q, n_feat, Sq, 0, Sq, flags);
    if (r) return r;
    if (ref0 > Sq) {
      r = pad_column(c, n_feat, Sq, flags);
      if (r) return r;
    }
    MatrixSrc ref = R;
    ref.dst_col = ref0;
    return icikt::host::upload_and_prepare(c, ref, n_feat, Sr, 0, Sr, flags);
  };
  return cross_run(call, Sq, Sr, A, blocks, upload);
}

// the device columns a reference of Sr columns with room for `capacity` query columns takes: the batch starts on an even
// column and may be followed by the partner of its last odd column in the interleaved tables
inline int64_t ref_total_cols(int64_t Sr, int64_t capacity) { return icikt::host::ref_query_col(Sr) + capacity + (capacity & 1); }

// icikt_ref_prepare_*: R is n_feat x Sr
int ref_prepare_src(icikt_ctx* c, const MatrixSrc& R, int64_t n_feat, int64_t Sr, int64_t capacity, const double* global_na,
                    int n_global_na, uint32_t flags) {
  if (!c) return ICIKT_E_INVALID;
  int rc = icikt::host::check_src(c, "ref_prepare", R, n_feat, Sr);
  if (rc) return rc;
  if (Sr < 1) return fail(c, ICIKT_E_INVALID, "ref_prepare: n_reference must be at least 1");
  if (capacity < 1)
    return fail(c, ICIKT_E_INVALID, "ref_prepare: query_capacity must be at least 1 (the room for a batch is allocated "
                                    "once; there is no unbounded capacity)");
  if (capacity > ICIKT_TOPK_MAX_SAMPLES || ref_total_cols(Sr, capacity) > ICIKT_TOPK_MAX_SAMPLES)
    return fail(c, ICIKT_E_INVALID, "ref_prepare: n_reference + query_capacity (+ 1 padding column for each that is odd) "
                                    "exceeds ICIKT_TOPK_MAX_SAMPLES (65535 columns: the pairs of a block are indexed in 32 bits)");
  icikt::MaskSpec ms;
  rc = icikt::host::make_mask_spec(c, global_na, n_global_na, &ms);
  if (!rc) rc = icikt::host::use_device(c);
  if (rc) return rc;
  const int64_t q0 = icikt::host::ref_query_col(Sr), total = ref_total_cols(Sr, capacity);
  const icikt::host::PinnedScope scope(c, flags);
  auto body = [&]() -> int {
    // d_X and the prepared state for ALL columns now: a DevBuf that grows drops what it holds, so a batch may not grow them
    HIPCHK(c, c->d_X.reserve((size_t)std::max<int64_t>(n_feat * total, 1)));
    int r = icikt::host::prepare_alloc(c, n_feat, total, total, total);
    if (r) return r;
    c->k0_mask = &ms;
    c->k0_keep = nullptr;
    r = icikt::host::upload_and_prepare(c, R, n_feat, Sr, 0, Sr, flags);
    if (!r && q0 > Sr) r = pad_column(c, n_feat, Sr, flags);
    return r;
  };
  rc = icikt::host::end_call(c, "ref_prepare", body());
  c->k0_mask = nullptr;
  icikt::host::forget_prepared(c);   // the device-resident calls start over: the tables are the reference's
  if (rc) return rc;
  // the tie verdict reads the first 64 prepared columns: reference columns, the same for every batch.  Settled here,
  // kept by icikt_ref_cross_* across its batches' pre-pass.
  c->pv.n_samp = (int)q0;
  icikt::host::settle_tie_verdict(c);
  c->ref.n_feat = n_feat;
  c->ref.n_reference = Sr;
  c->ref.capacity = capacity;
  c->ref.ms = ms;
  c->ref.valid = true;
  return ICIKT_SUCCESS;
}

// icikt_ref_cross_*: Q is n_feat x Sq, against the context's prepared reference
int ref_cross_src(icikt_ctx* c, const MatrixSrc& Q, int64_t n_feat, int64_t Sq, const CrossArgs& A) {
  if (!c) return ICIKT_E_INVALID;
  if (!c->ref.valid)
    return fail(c, ICIKT_E_STATE, "ref_cross: the context holds no prepared reference (icikt_ref_prepare_f64 has not been "
                                  "called, or a later call has replaced the prepared state)");
  icikt::host::SelectCall call{c, "ref_cross", Q, n_feat, Sq, A.shared, {}};
  int rc = icikt::host::check_src(c, "ref_cross (query)", Q, n_feat, Sq);
  if (rc) return rc;
  const int64_t Sr = c->ref.n_reference;
  if (n_feat != c->ref.n_feat)
    return fail(c, ICIKT_E_INVALID, "ref_cross: n_feat = " + std::to_string(n_feat) + ", the prepared reference has " +
                                        std::to_string(c->ref.n_feat) + " rows");
  if (Sq > c->ref.capacity)
    return fail(c, ICIKT_E_INVALID, "ref_cross: n_query = " + std::to_string(Sq) + " exceeds the query_capacity the reference "
                                        "was prepared with (" + std::to_string(c->ref.capacity) + "): split the batch");
  rc = cross_check_outputs(c, "ref_cross", A, Sr);
  if (!rc) rc = icikt::host::select_check_args(call);
  if (rc) return rc;
  call.ms = c->ref.ms;   // the rule the reference was pre-passed under
  if (Sq == 0) {
    cross_empty(A, Sq);
    return ICIKT_SUCCESS;
  }
  int64_t budget;
  rc = icikt::host::select_budget(call, &budget);
  if (rc) return rc;
  PairBlocks blocks = PairBlocks::rect_ref_first(Sq, Sr, budget);
  const int64_t q0 = icikt::host::ref_query_col(Sr);
  const uint32_t flags = A.shared.flags;
  const std::function<int()> upload = [&]() -> int {
    // no prepare_alloc, no reserve that could grow: the batch's columns land in the room ref_prepare allocated
    c->k0_mask = &call.ms;
    c->k0_keep = nullptr;
    c->pv.n_samp = (int)(q0 + Sq);
    const int tied = c->tied_state, ntg = c->ntg_hint, group = c->group_hint;   // (prepare_launch resets them)
    MatrixSrc q = Q;
    q.dst_col = q0;
    const int r = icikt::host::upload_and_prepare(c, q, n_feat, Sq, 0, Sq, flags);
    c->tied_state = tied;
    c->ntg_hint = ntg;
    c->group_hint = group;
    return r;
  };
  rc = cross_run(call, Sq, Sr, A, blocks, upload);
  // select_run has forgotten the pair list and the batch; the reference's tables were not written
  c->ref.valid = rc == ICIKT_SUCCESS;
  return rc;
}

}  // namespace

#define CROSS_SHARED {global_na, n_global_na, perspective, alternative, continuity, flags, max_taumax, reason_counts}
#define CROSS_ARGS CrossArgs{CROSS_SHARED, k, scale_max, out5, idx, out5k, n_valid, nullptr, 0, nullptr, nullptr}
#define REF_CROSS_ARGS CrossArgs{{nullptr, 0, perspective, alternative, continuity, flags, max_taumax, reason_counts}, \
                                 k, scale_max, out5, idx, out5k, n_valid, ref_cls, n_class, cls_med2, cls_n_valid}

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

int icikt_ref_prepare_f64(icikt_ctx* c, const double* R, int64_t ld_reference, int64_t n_feat, int64_t n_reference,
                          int64_t query_capacity, const double* global_na, int n_global_na, uint32_t flags) {
  const icikt_input r = icikt::host::f64_view(R, ld_reference);
  return ref_prepare_src(c, MatrixSrc::dense(&r), n_feat, n_reference, query_capacity, global_na, n_global_na, flags);
}

int icikt_ref_prepare_in(icikt_ctx* c, const icikt_input* R, int64_t n_feat, int64_t n_reference, int64_t query_capacity,
                         const double* global_na, int n_global_na, uint32_t flags) {
  return ref_prepare_src(c, MatrixSrc::dense(R), n_feat, n_reference, query_capacity, global_na, n_global_na, flags);
}

int icikt_ref_cross_f64(icikt_ctx* c, const double* Q, int64_t ld_query, int64_t n_feat, int64_t n_query, int k,
                        const int32_t* ref_cls, int n_class, int perspective, int alternative, int continuity,
                        uint32_t flags, int scale_max, double* out5, int32_t* idx, double* out5k, int32_t* n_valid,
                        double* cls_med2, int32_t* cls_n_valid, double* max_taumax, int64_t* reason_counts) {
  const icikt_input q = icikt::host::f64_view(Q, ld_query);
  return ref_cross_src(c, MatrixSrc::dense(&q), n_feat, n_query, REF_CROSS_ARGS);
}

int icikt_ref_cross_in(icikt_ctx* c, const icikt_input* Q, int64_t n_feat, int64_t n_query, int k, const int32_t* ref_cls,
                       int n_class, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                       double* out5, int32_t* idx, double* out5k, int32_t* n_valid, double* cls_med2,
                       int32_t* cls_n_valid, double* max_taumax, int64_t* reason_counts) {
  return ref_cross_src(c, MatrixSrc::dense(Q), n_feat, n_query, REF_CROSS_ARGS);
}

int icikt_ref_info(icikt_ctx* c, int64_t* n_feat, int64_t* n_reference, int64_t* query_capacity) {
  if (!c) return ICIKT_E_INVALID;
  if (!c->ref.valid) return fail(c, ICIKT_E_STATE, "ref_info: the context holds no prepared reference");
  if (n_feat) *n_feat = c->ref.n_feat;
  if (n_reference) *n_reference = c->ref.n_reference;
  if (query_capacity) *query_capacity = c->ref.capacity;
  return ICIKT_SUCCESS;
}

}  // extern "C"
