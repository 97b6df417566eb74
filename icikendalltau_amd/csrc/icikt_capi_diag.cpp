// icikt_capi_diag.cpp -- the C-ABI entries of the missing-value diagnostics (icikt_col_medians_f64,
// icikt_censor_counts_f64, icikt_rank_order_f64), sequencing the kernels of icikt_diag.hip on a context's stream.
// The context, the entry checks and the timers they share with the pair engine are in icikt_capi.cpp (declared in
// icikt_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::host::f64_view;
using icikt::host::fail;
using icikt::host::MatrixSrc;
using icikt::host::timer_begin;
using icikt::host::timer_end;
using icikt::host::use_device;

// ---- missing-value diagnostics (R/left_censorship.R, R/rank-ordering.R) ----
// Timers: K_PREPARE the matrix's H2D, K_PAIRS the column and row passes, K_EPILOGUE the orders and the gathers.
namespace {

// the per-column pass over the device matrix dX (n x S, leading dimension n); rank mode when kept != nullptr
int diag_col_pass(icikt_ctx* c, const double* dX, int64_t n, int64_t S, const icikt::MaskSpec& ms, int na_rm,
                  const uint8_t* kept, int32_t* rank2) {
  icikt_ctx::DiagBufs& db = c->diag;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>({S, 2048,
      std::max<int64_t>(1, ((int64_t)1 << 29) / ((int64_t)np2 * 16))}));
  const size_t scratch = (size_t)blocks * (size_t)np2;
  const size_t nS = (size_t)std::max<int64_t>(S, 1);
  HIPCHK(c, db.keys.reserve(scratch));
  HIPCHK(c, db.idx.reserve(scratch));
  HIPCHK(c, db.gs.reserve(scratch));
  HIPCHK(c, db.median.reserve(nS));
  HIPCHK(c, db.nmiss.reserve(nS));
  HIPCHK(c, db.nexcl.reserve(nS));
  icikt::DiagCol dc{};
  dc.X = dX;
  dc.ld = n;
  dc.n = n;
  dc.S = (int)S;
  dc.ms = ms;
  dc.na_rm = na_rm;
  dc.median = db.median.p;
  dc.nmiss = db.nmiss.p;
  dc.nexcl = db.nexcl.p;
  dc.kept = kept;
  dc.rank2 = rank2;
  dc.keys = reinterpret_cast<uint64_t*>(db.keys.p);
  dc.idx = db.idx.p;
  dc.gs = db.gs.p;
  dc.np2 = np2;
  HIPCHK(c, icikt::launch_diag_col(dc, blocks, c->stream));
  return ICIKT_SUCCESS;
}

// shape, matrix, global_na of the three entries; sets *ms
int diag_args(icikt_ctx* c, const char* who, const MatrixSrc& X, int64_t n_feat, int64_t n_samp,
              const double* global_na, int n_global_na, icikt::MaskSpec* ms) {
  int rc = icikt::host::check_src(c, who, X, n_feat, n_samp);
  if (rc) return rc;
  if (n_samp > INT32_MAX) return fail(c, ICIKT_E_INVALID, std::string(who) + ": too many columns");
  rc = icikt::host::make_mask_spec(c, global_na, n_global_na, ms);
  if (rc) c->err = std::string(who) + c->err.substr(c->err.find(':'));
  return rc;
}

// the bodies the _in and _csc entries share
int col_medians_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, int na_rm, uint32_t flags, double* medians);
int censor_counts_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                      int n_global_na, const int32_t* cls, int n_class, uint32_t flags, int64_t* trials, int64_t* success,
                      int64_t* n_excluded, double* medians);
int rank_order_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, const int32_t* cols, int64_t n_cols, uint32_t flags, int64_t* n_kept, int32_t* n_na,
                   double* median_rank, int32_t* row_order, int32_t* col_order, double* original, double* ordered);

}  // namespace

extern "C" {

int icikt_col_medians_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                          const double* global_na, int n_global_na, int na_rm, uint32_t flags, double* medians) {
  const icikt_input v = f64_view(X, ld);
  return icikt_col_medians_in(c, &v, n_feat, n_samp, global_na, n_global_na, na_rm, flags, medians);
}

int icikt_col_medians_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                         int n_global_na, int na_rm, uint32_t flags, double* medians) {
  return col_medians_src(c, MatrixSrc::dense(X), n_feat, n_samp, global_na, n_global_na, na_rm, flags, medians);
}

int icikt_col_medians_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp,
                          const double* global_na, int n_global_na, int na_rm, uint32_t flags, double* medians) {
  return col_medians_src(c, MatrixSrc::csc(X), n_feat, n_samp, global_na, n_global_na, na_rm, flags, medians);
}

}  // extern "C"

namespace {

int col_medians_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, int na_rm, uint32_t flags, double* medians) {
  if (!c) return ICIKT_E_INVALID;
  icikt::MaskSpec ms;
  int rc = diag_args(c, "col_medians", X, n_feat, n_samp, global_na, n_global_na, &ms);
  if (rc) return rc;
  if (n_samp == 0) return ICIKT_SUCCESS;
  if (!medians) return fail(c, ICIKT_E_INVALID, "col_medians: null output");
  rc = use_device(c);
  if (rc) return rc;
  const icikt::host::PinnedScope scope(c, flags);
  auto body = [&]() -> int {
    int r = icikt::host::upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags, false, nullptr,
                                            icikt::host::kPrepassNone);
    if (!r) r = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (!r) r = diag_col_pass(c, c->d_X.p, n_feat, n_samp, ms, na_rm, nullptr, nullptr);
    if (!r) r = timer_end(c, ICIKT_K_PAIRS, flags);
    if (!r) r = icikt::host::download(c, medians, c->diag.median.p, (size_t)n_samp * sizeof(double));
    return r;
  };
  return icikt::host::end_call(c, "col_medians", body());
}

}  // namespace

extern "C" {

int icikt_censor_counts_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                            const double* global_na, int n_global_na, const int32_t* cls, int n_class, uint32_t flags,
                            int64_t* trials, int64_t* success, int64_t* n_excluded, double* medians) {
  const icikt_input v = f64_view(X, ld);
  return icikt_censor_counts_in(c, &v, n_feat, n_samp, global_na, n_global_na, cls, n_class, flags, trials, success,
                                n_excluded, medians);
}

int icikt_censor_counts_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                           int n_global_na, const int32_t* cls, int n_class, uint32_t flags, int64_t* trials,
                           int64_t* success, int64_t* n_excluded, double* medians) {
  return censor_counts_src(c, MatrixSrc::dense(X), n_feat, n_samp, global_na, n_global_na, cls, n_class, flags, trials,
                           success, n_excluded, medians);
}

int icikt_censor_counts_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp,
                            const double* global_na, int n_global_na, const int32_t* cls, int n_class, uint32_t flags,
                            int64_t* trials, int64_t* success, int64_t* n_excluded, double* medians) {
  return censor_counts_src(c, MatrixSrc::csc(X), n_feat, n_samp, global_na, n_global_na, cls, n_class, flags, trials,
                           success, n_excluded, medians);
}

}  // extern "C"

namespace {

int censor_counts_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                      int n_global_na, const int32_t* cls, int n_class, uint32_t flags, int64_t* trials, int64_t* success,
                      int64_t* n_excluded, double* medians) {
  if (!c) return ICIKT_E_INVALID;
  icikt::MaskSpec ms;
  int rc = diag_args(c, "censor_counts", X, n_feat, n_samp, global_na, n_global_na, &ms);
  if (rc) return rc;
  if (n_class < 1) return fail(c, ICIKT_E_INVALID, "censor_counts: n_class must be at least 1");
  if (n_samp > 0 && !cls) return fail(c, ICIKT_E_INVALID, "censor_counts: null class list");
  if (!trials || !success || !n_excluded) return fail(c, ICIKT_E_INVALID, "censor_counts: null output");
  // the columns grouped by class, in column order within a class
  std::vector<int32_t> off((size_t)n_class + 1, 0), cols((size_t)n_samp);
  for (int64_t j = 0; j < n_samp; ++j) {
    if (cls[j] < 0 || cls[j] >= n_class) return fail(c, ICIKT_E_INVALID, "censor_counts: class index out of range");
    ++off[(size_t)cls[j] + 1];
  }
  for (int k = 0; k < n_class; ++k) off[(size_t)k + 1] += off[(size_t)k];
  {
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (int64_t j = 0; j < n_samp; ++j) cols[(size_t)fill[(size_t)cls[j]]++] = (int32_t)j;
  }
  for (int k = 0; k < n_class; ++k) trials[k] = success[k] = 0;
  *n_excluded = 0;
  if (n_samp == 0) return ICIKT_SUCCESS;
  rc = use_device(c);
  if (rc) return rc;
  const icikt::host::PinnedScope scope(c, flags);
  icikt_ctx::DiagBufs& db = c->diag;
  std::vector<unsigned long long> out3((size_t)n_class * 3);
  std::vector<int32_t> nexcl((size_t)n_samp);
  auto body = [&]() -> int {
    int r = icikt::host::upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, flags, false, nullptr,
                                            icikt::host::kPrepassNone);
    if (r) return r;
    HIPCHK(c, db.lists.reserve(off.size() + cols.size()));
    HIPCHK(c, db.red.reserve(out3.size()));
    r = icikt::host::upload_sync(c, db.lists.p, off.data(), off.size() * sizeof(int32_t));
    if (!r) r = icikt::host::upload_sync(c, db.lists.p + off.size(), cols.data(), cols.size() * sizeof(int32_t));
    if (!r) r = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(db.red.p, 0, out3.size() * sizeof(unsigned long long), c->stream));
    r = diag_col_pass(c, c->d_X.p, n_feat, n_samp, ms, 1, nullptr, nullptr);
    if (r) return r;
    HIPCHK(c, icikt::launch_diag_censor(c->d_X.p, n_feat, n_feat, ms, db.lists.p + off.size(), db.lists.p, n_class,
                                        db.median.p, db.red.p, c->stream));
    r = timer_end(c, ICIKT_K_PAIRS, flags);
    if (!r) r = icikt::host::download(c, out3.data(), db.red.p, out3.size() * sizeof(unsigned long long));
    if (!r) r = icikt::host::download(c, nexcl.data(), db.nexcl.p, nexcl.size() * sizeof(int32_t));
    if (!r && medians) r = icikt::host::download(c, medians, db.median.p, (size_t)n_samp * sizeof(double));
    return r;
  };
  rc = icikt::host::end_call(c, "censor_counts", body());
  if (rc) return rc;
  for (int k = 0; k < n_class; ++k) {
    trials[k] = (int64_t)out3[3 * (size_t)k];
    success[k] = (int64_t)out3[3 * (size_t)k + 1];
  }
  int64_t ex = 0;
  for (int32_t v : nexcl) ex += v;
  *n_excluded = ex;
  return ICIKT_SUCCESS;
}

}  // namespace

extern "C" {

int icikt_rank_order_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                         const double* global_na, int n_global_na, const int32_t* cols, int64_t n_cols, uint32_t flags,
                         int64_t* n_kept, int32_t* n_na, double* median_rank, int32_t* row_order, int32_t* col_order,
                         double* original, double* ordered) {
  const icikt_input v = f64_view(X, ld);
  return icikt_rank_order_in(c, &v, n_feat, n_samp, global_na, n_global_na, cols, n_cols, flags, n_kept, n_na, median_rank,
                             row_order, col_order, original, ordered);
}

int icikt_rank_order_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                        int n_global_na, const int32_t* cols, int64_t n_cols, uint32_t flags, int64_t* n_kept,
                        int32_t* n_na, double* median_rank, int32_t* row_order, int32_t* col_order, double* original,
                        double* ordered) {
  return rank_order_src(c, MatrixSrc::dense(X), n_feat, n_samp, global_na, n_global_na, cols, n_cols, flags, n_kept, n_na,
                        median_rank, row_order, col_order, original, ordered);
}

int icikt_rank_order_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp,
                         const double* global_na, int n_global_na, const int32_t* cols, int64_t n_cols, uint32_t flags,
                         int64_t* n_kept, int32_t* n_na, double* median_rank, int32_t* row_order, int32_t* col_order,
                         double* original, double* ordered) {
  return rank_order_src(c, MatrixSrc::csc(X), n_feat, n_samp, global_na, n_global_na, cols, n_cols, flags, n_kept, n_na,
                        median_rank, row_order, col_order, original, ordered);
}

}  // extern "C"

namespace {

int rank_order_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                   int n_global_na, const int32_t* cols, int64_t n_cols, uint32_t flags, int64_t* n_kept, int32_t* n_na,
                   double* median_rank, int32_t* row_order, int32_t* col_order, double* original, double* ordered) {
  if (!c) return ICIKT_E_INVALID;
  icikt::MaskSpec ms;
  int rc = diag_args(c, "rank_order", X, n_feat, n_samp, global_na, n_global_na, &ms);
  if (rc) return rc;
  if (n_cols < 1 || n_cols > n_samp || !cols) return fail(c, ICIKT_E_INVALID, "rank_order: bad column list");
  for (int64_t j = 0; j < n_cols; ++j)
    if (cols[j] < 0 || cols[j] >= n_samp) return fail(c, ICIKT_E_INVALID, "rank_order: column index out of range");
  if (!n_kept || (n_feat > 0 && (!n_na || !median_rank || !row_order)) || !col_order)
    return fail(c, ICIKT_E_INVALID, "rank_order: null output");
  *n_kept = 0;
  rc = use_device(c);
  if (rc) return rc;
  const int64_t n = n_feat;
  // the class's columns as one block: in place when they are consecutive (the view from column cols[0] on, in either
  // order), else gathered on the host in the view's element type, column-major (one pass)
  bool consecutive = true;
  for (int64_t j = 1; j < n_cols && consecutive; ++j) consecutive = cols[j] == cols[0] + j;
  std::vector<char> gathered, gathered_idx, gathered_ptr;
  bool copied = false;   // the block is a copy of this function's: pageable, whatever the caller says about ITS memory
  MatrixSrc src = X;
  if (X.sparse) {
    // consecutive columns: the same values / indices behind indptr + cols[0]; else slices of values / indices, column by
    // column, and a rebuilt indptr -- O(entries of the listed columns)
    const icikt_csc_input& s = X.s;
    const size_t es = icikt::host::dtype_bytes(s.dtype), is = icikt::host::index_bytes(s.index_type);
    if (consecutive) {
      src.s.indptr = static_cast<const char*>(s.indptr) + (size_t)cols[0] * is;
    } else {
      size_t total = 0;
      for (int64_t j = 0; j < n_cols; ++j) total += (size_t)(icikt::host::csc_ptr(s, cols[j] + 1) - icikt::host::csc_ptr(s, cols[j]));
      gathered.resize(total * es);
      gathered_idx.resize(total * is);
      gathered_ptr.resize((size_t)(n_cols + 1) * is);
      size_t at = 0;
      auto put = [&](int64_t j, size_t v) {
        if (is == 8) reinterpret_cast<int64_t*>(gathered_ptr.data())[j] = (int64_t)v;
        else reinterpret_cast<int32_t*>(gathered_ptr.data())[j] = (int32_t)v;
      };
      for (int64_t j = 0; j < n_cols; ++j) {
        const int64_t e0 = icikt::host::csc_ptr(s, cols[j]), cnt = icikt::host::csc_ptr(s, cols[j] + 1) - e0;
        put(j, at);
        if (cnt > 0) {
          std::memcpy(gathered.data() + at * es, static_cast<const char*>(s.values) + (size_t)e0 * es, (size_t)cnt * es);
          std::memcpy(gathered_idx.data() + at * is, static_cast<const char*>(s.indices) + (size_t)e0 * is, (size_t)cnt * is);
        }
        at += (size_t)cnt;
      }
      put(n_cols, at);
      src.s.values = gathered.data();
      src.s.indices = gathered_idx.data();
      src.s.indptr = gathered_ptr.data();
      copied = true;
    }
  } else {
  src = MatrixSrc(n > 0 ? icikt::host::view_from_col(X.v, cols[0]) : X.v);
  if (!consecutive && n > 0) {
    const icikt_input* Xv = &X.v;
    const size_t es = icikt::host::dtype_bytes(Xv->dtype);
    gathered.resize((size_t)n * (size_t)n_cols * es);
    const char* base = static_cast<const char*>(Xv->data);
    for (int64_t j = 0; j < n_cols; ++j) {
      char* dstc = gathered.data() + (size_t)j * (size_t)n * es;
      if (Xv->order == ICIKT_ORDER_COL) {
        std::memcpy(dstc, base + (size_t)cols[j] * (size_t)Xv->ld * es, (size_t)n * es);
      } else {
        const char* s0 = base + (size_t)cols[j] * es;
        const size_t step = (size_t)Xv->ld * es;
        if (es == 4) for (int64_t r = 0; r < n; ++r) std::memcpy(dstc + 4 * (size_t)r, s0 + (size_t)r * step, 4);
        else for (int64_t r = 0; r < n; ++r) std::memcpy(dstc + 8 * (size_t)r, s0 + (size_t)r * step, 8);
      }
    }
    src = MatrixSrc(icikt_input{gathered.data(), Xv->dtype, ICIKT_ORDER_COL, n});
    copied = true;
  }
  }
  const icikt::host::PinnedScope scope(c, copied ? (flags & ~ICIKT_FLAG_HOST_PINNED) : flags);
  icikt_ctx::DiagBufs& db = c->diag;
  std::vector<int32_t> nmiss((size_t)n_cols);
  unsigned long long kept_count = 0;
  // device passes, then the counts and medians back to the host
  auto passes = [&]() -> int {
    int r = icikt::host::upload_and_prepare(c, src, n, n_cols, 0, n_cols, flags, false, nullptr,
                                            icikt::host::kPrepassNone);
    if (r) return r;
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    HIPCHK(c, db.kept.reserve(nn));
    HIPCHK(c, db.nna.reserve(nn));
    HIPCHK(c, db.medrank.reserve(nn));
    HIPCHK(c, db.rank2.reserve(nn * (size_t)n_cols));
    HIPCHK(c, db.red.reserve(1));
    r = timer_begin(c, ICIKT_K_PAIRS, flags);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(db.red.p, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, icikt::launch_diag_rowmiss(c->d_X.p, n, (int)n_cols, ms, db.nna.p, db.kept.p, db.red.p, c->stream));
    r = diag_col_pass(c, c->d_X.p, n, n_cols, ms, 1, db.kept.p, db.rank2.p);
    if (r) return r;
    HIPCHK(c, icikt::launch_diag_median_rank(db.rank2.p, n, (int)n_cols, db.kept.p, db.medrank.p, c->stream));
    r = timer_end(c, ICIKT_K_PAIRS, flags);
    if (!r) r = icikt::host::download(c, &kept_count, db.red.p, sizeof(unsigned long long));
    if (!r) r = icikt::host::download(c, nmiss.data(), db.nmiss.p, nmiss.size() * sizeof(int32_t));
    if (!r && n > 0) r = icikt::host::download(c, n_na, db.nna.p, (size_t)n * sizeof(int32_t));
    if (!r && n > 0) r = icikt::host::download(c, median_rank, db.medrank.p, (size_t)n * sizeof(double));
    if (r) return r;
    const hipError_t e = icikt::host::finish_stream(c, true);
    if (e != hipSuccess) return fail(c, ICIKT_E_HIP, std::string("rank_order: ") + hipGetErrorString(e));
    return ICIKT_SUCCESS;
  };
  rc = passes();
  if (rc) return icikt::host::end_call(c, "rank_order", rc);
  const int64_t nk = (int64_t)kept_count;
  // order(median_rank, decreasing = TRUE) over the kept rows, order(colMeans(is.na), decreasing = TRUE): both stable.
  // (The dropped rows are missing in every column: they shift every column's count alike.)
  std::vector<int32_t> kept_rows;
  kept_rows.reserve((size_t)nk);
  for (int64_t r = 0; r < n; ++r)
    if (n_na[r] < n_cols) kept_rows.push_back((int32_t)r);
  if ((int64_t)kept_rows.size() != nk) return icikt::host::end_call(c, "rank_order",
      fail(c, ICIKT_E_HIP, "rank_order: kept-row count differs between device and host"));
  std::vector<int32_t> rord(kept_rows);
  std::stable_sort(rord.begin(), rord.end(), [&](int32_t a, int32_t b) { return median_rank[a] > median_rank[b]; });
  std::vector<int32_t> cord((size_t)n_cols);
  for (int64_t j = 0; j < n_cols; ++j) cord[(size_t)j] = (int32_t)j;
  std::stable_sort(cord.begin(), cord.end(), [&](int32_t a, int32_t b) { return nmiss[(size_t)a] > nmiss[(size_t)b]; });
  std::copy(rord.begin(), rord.end(), row_order);
  std::copy(cord.begin(), cord.end(), col_order);
  *n_kept = nk;
  auto gathers = [&]() -> int {
    if (nk == 0 || (!original && !ordered)) return ICIKT_SUCCESS;
    std::vector<int32_t> lists;   // kept rows | row order | identity columns | column order
    lists.reserve(2 * (size_t)nk + 2 * (size_t)n_cols);
    lists.insert(lists.end(), kept_rows.begin(), kept_rows.end());
    lists.insert(lists.end(), rord.begin(), rord.end());
    for (int64_t j = 0; j < n_cols; ++j) lists.push_back((int32_t)j);
    lists.insert(lists.end(), cord.begin(), cord.end());
    HIPCHK(c, db.lists.reserve(lists.size()));
    int r = icikt::host::upload_sync(c, db.lists.p, lists.data(), lists.size() * sizeof(int32_t));
    if (r) return r;
    const size_t cells = (size_t)nk * (size_t)n_cols;
    HIPCHK(c, db.out.reserve(2 * cells));
    r = timer_begin(c, ICIKT_K_EPILOGUE, flags);
    if (r) return r;
    const int32_t* d_kept = db.lists.p;
    const int32_t* d_rord = d_kept + nk;
    const int32_t* d_cid = d_rord + nk;
    const int32_t* d_cord = d_cid + n_cols;
    if (original)
      HIPCHK(c, icikt::launch_diag_gather(c->d_X.p, n, ms, d_kept, nk, d_cid, (int)n_cols, db.out.p, c->stream));
    if (ordered)
      HIPCHK(c, icikt::launch_diag_gather(c->d_X.p, n, ms, d_rord, nk, d_cord, (int)n_cols, db.out.p + cells, c->stream));
    r = timer_end(c, ICIKT_K_EPILOGUE, flags);
    if (!r && original) r = icikt::host::download(c, original, db.out.p, cells * sizeof(double));
    if (!r && ordered) r = icikt::host::download(c, ordered, db.out.p + cells, cells * sizeof(double));
    return r;
  };
  return icikt::host::end_call(c, "rank_order", gathers());
}

}  // namespace
