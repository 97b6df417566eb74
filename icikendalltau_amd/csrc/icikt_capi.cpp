// icikt_capi.cpp -- host side of the C ABI declared in include/icikt.h: the pair engine's entries.
//
// Owns the HIP device/stream/workspaces of a context: its life cycle, the timers, the argument checks, the prepare /
// run / pairs / matrix / complete / missingness entries, the debug hooks and the self-test.  What enqueues copies, the
// pre-pass (icikt_prepass.hip) and the pair kernels (icikt_kernels.hip) for them is in icikt_pipeline.cpp; the epilogue
// and assembly (icikt_epilogue.hip) are launched here.  cor_fast's entry is in icikt_capi_cor.cpp, the missing-value
// diagnostics' in icikt_capi_diag.cpp.  There is deliberately NO CPU implementation of the arithmetic here: when no
// HIP device is usable every entry point fails with ICIKT_E_NO_DEVICE / ICIKT_E_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "icikt.h"
#include "icikt_device.h"
#include "icikt_host.h"

using icikt::PrepView;

static_assert(ICIKT_CNT_FIELDS == icikt::ICIKT_CNT_FIELDS_, "counts record layout");
static_assert(ICIKT_PERSPECTIVE_LOCAL == icikt::ICIKT_PERSPECTIVE_LOCAL_, "perspective code");

namespace {

// fold the recorded event pairs of kernel k into the accumulated time (waits for them to complete)
int flush_timer(icikt_ctx* c, int k) {
  for (size_t i = 0; i < c->ev_used[k]; ++i) {
    HIPCHK(c, hipEventSynchronize(c->ev_pool[k][i].b));
    float t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&t, c->ev_pool[k][i].a, c->ev_pool[k][i].b));
    c->ms[k] += (double)t;
    c->launches[k] += 1;
  }
  c->ev_used[k] = 0;
  return ICIKT_SUCCESS;
}

}  // namespace

namespace icikt {
namespace host {

int fail(icikt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

int use_device(icikt_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  return ICIKT_SUCCESS;
}

int timer_begin(icikt_ctx* c, int k, uint32_t flags) {
  if (!(flags & ICIKT_FLAG_TIMING)) return ICIKT_SUCCESS;
  if (c->ev_used[k] == c->ev_pool[k].size()) {
    if (c->ev_pool[k].size() >= 256) {  // pool full: the one place a timed launch waits for earlier ones
      int rc = flush_timer(c, k);
      if (rc) return rc;
    } else {
      icikt_ctx::EvPair p;
      HIPCHK(c, hipEventCreate(&p.a));
      HIPCHK(c, hipEventCreate(&p.b));
      c->ev_pool[k].push_back(p);
    }
  }
  HIPCHK(c, hipEventRecord(c->ev_pool[k][c->ev_used[k]].a, c->stream));
  c->ev_open[k] = true;
  return ICIKT_SUCCESS;
}

int timer_end(icikt_ctx* c, int k, uint32_t flags) {
  if (!(flags & ICIKT_FLAG_TIMING) || !c->ev_open[k]) return ICIKT_SUCCESS;
  HIPCHK(c, hipEventRecord(c->ev_pool[k][c->ev_used[k]].b, c->stream));
  c->ev_used[k] += 1;
  c->ev_open[k] = false;
  return ICIKT_SUCCESS;
}

}  // namespace host
}  // namespace icikt

using icikt::host::fail;
using icikt::host::use_device;
using icikt::host::timer_begin;
using icikt::host::timer_end;

extern "C" {

int icikt_version(void) { return ICIKT_VERSION; }

int icikt_device_count(int* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  if (count) *count = n;
  return n > 0 ? ICIKT_SUCCESS : ICIKT_E_NO_DEVICE;
}

int icikt_ctx_create(int device, icikt_ctx** out) {
  if (!out) return ICIKT_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ICIKT_E_NO_DEVICE;
  if (device < 0 || device >= n) return ICIKT_E_INVALID;
  icikt_ctx* c = new (std::nothrow) icikt_ctx();
  if (!c) return ICIKT_E_NOMEM;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return ICIKT_E_HIP;
  }
  c->stream = c->own_stream;
  // the pre-pass of a chunk must not queue behind the pair kernel of the chunks before it for longer than that
  // kernel's workgroups take to retire: the highest priority the device offers
  int lo_prio = 0, hi_prio = 0;
  if (hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio) != hipSuccess) { (void)hipGetLastError(); hi_prio = 0; }
  if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&c->prep_stream, hipStreamNonBlocking, hi_prio) != hipSuccess || c->xfer.init() != hipSuccess) {
    icikt_ctx_destroy(c);
    return ICIKT_E_HIP;
  }
  *out = c;
  return ICIKT_SUCCESS;
}

void icikt_ctx_destroy(icikt_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  for (int k = 0; k < ICIKT_K_COUNT; ++k)
    for (auto& p : c->ev_pool[k]) {
      if (p.a) (void)hipEventDestroy(p.a);
      if (p.b) (void)hipEventDestroy(p.b);
    }
  for (auto& e : c->ev_chunk)
    if (e) (void)hipEventDestroy(e);
  if (c->prep_stream) { (void)hipStreamSynchronize(c->prep_stream); (void)hipStreamDestroy(c->prep_stream); }
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;   // (the device buffers, and the transfers' pinned buffers, threads and events, go with it)
}

const char* icikt_last_error(const icikt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int icikt_ctx_set_stream(icikt_ctx* c, void* hip_stream) {
  if (!c) return ICIKT_E_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  (void)hipStreamSynchronize(c->stream);
  c->stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL is HIP's default (null) stream
  return ICIKT_SUCCESS;
}

int icikt_ctx_use_own_stream(icikt_ctx* c) {
  if (!c) return ICIKT_E_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  (void)hipStreamSynchronize(c->stream);
  c->stream = c->own_stream;
  return ICIKT_SUCCESS;
}

int icikt_sync(icikt_ctx* c) {
  if (!c) return ICIKT_E_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ICIKT_SUCCESS;
}

}  // extern "C"

// Shared body of icikt_prepare_dev / icikt_prepare_cols_dev: allocate the prepared state for alloc_cols
// columns and run the pre-pass over columns [col_begin, col_end).
static const char* const kTooLong =
    "n_feat exceeds ICIKT_MAX_FEATURES_WIDE (262144 rows per column; the tuned kernels take up to 65535, the plain "
    "32-bit path up to 262144 -- its bitsets must fit the LDS of a CU)";
static const char* const kNoWide =
    "n_feat exceeds ICIKT_MAX_FEATURES (65535 rows per column): this entry has no path for wide columns";

namespace icikt {
namespace host {

int check_shape(icikt_ctx* c, const char* who, int64_t n_feat, int64_t n_samp, int64_t ld, bool wide_ok) {
  if (n_feat < 0 || n_samp < 0 || ld < n_feat) return fail(c, ICIKT_E_INVALID, std::string(who) + ": bad matrix shape (n_feat, n_samp or ld)");
  if (n_feat > ICIKT_MAX_FEATURES_WIDE) return fail(c, ICIKT_E_TOO_LONG, std::string(who) + ": " + kTooLong);
  if (n_feat > ICIKT_MAX_FEATURES && !wide_ok) return fail(c, ICIKT_E_TOO_LONG, std::string(who) + ": " + kNoWide);
  return ICIKT_SUCCESS;
}

int check_view(icikt_ctx* c, const char* who, const icikt_input* X, int64_t n_feat, int64_t n_samp, bool wide_ok) {
  const std::string w(who);
  if (!X) return fail(c, ICIKT_E_INVALID, w + ": X is null (the icikt_input view of the matrix)");
  if (X->dtype < ICIKT_DTYPE_F64 || X->dtype > ICIKT_DTYPE_I64)
    return fail(c, ICIKT_E_INVALID, w + ": X->dtype must be one of ICIKT_DTYPE_F64, _F32, _I32, _I64");
  if (X->order != ICIKT_ORDER_COL && X->order != ICIKT_ORDER_ROW)
    return fail(c, ICIKT_E_INVALID, w + ": X->order must be ICIKT_ORDER_COL or ICIKT_ORDER_ROW");
  const bool row = X->order == ICIKT_ORDER_ROW;
  if (row && n_feat >= 0 && n_samp >= 0 && X->ld < n_samp)
    return fail(c, ICIKT_E_INVALID, w + ": bad matrix shape (X->ld is below n_samp, the row of a row-major view)");
  const int rc = check_shape(c, who, n_feat, n_samp, row ? n_feat : X->ld, wide_ok);
  if (rc) return rc;
  if (n_feat > 0 && n_samp > 0 && !X->data) return fail(c, ICIKT_E_INVALID, w + ": null matrix");
  return ICIKT_SUCCESS;
}

int check_src(icikt_ctx* c, const char* who, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, bool wide_ok) {
  if (!X.sparse) return check_view(c, who, X.null ? nullptr : &X.v, n_feat, n_samp, wide_ok);
  const std::string w(who);
  if (X.null) return fail(c, ICIKT_E_INVALID, w + ": X is null (the icikt_csc_input view of the matrix)");
  const icikt_csc_input& s = X.s;
  if (s.dtype < ICIKT_DTYPE_F64 || s.dtype > ICIKT_DTYPE_I64)
    return fail(c, ICIKT_E_INVALID, w + ": X->dtype must be one of ICIKT_DTYPE_F64, _F32, _I32, _I64");
  if (s.index_type != ICIKT_INDEX_I32 && s.index_type != ICIKT_INDEX_I64)
    return fail(c, ICIKT_E_INVALID, w + ": X->index_type must be ICIKT_INDEX_I32 or ICIKT_INDEX_I64");
  const int rc = check_shape(c, who, n_feat, n_samp, n_feat, wide_ok);
  if (rc) return rc;
  if (!s.indptr) return fail(c, ICIKT_E_INVALID, w + ": X->indptr is null (n_samp + 1 column offsets)");
  if (csc_ptr(s, 0) < 0) return fail(c, ICIKT_E_INVALID, w + ": X->indptr[0] is negative");
  for (int64_t j = 0; j < n_samp; ++j)
    if (csc_ptr(s, j + 1) < csc_ptr(s, j))
      return fail(c, ICIKT_E_INVALID, w + ": X->indptr decreases at column " + std::to_string((long long)j));
  if (csc_ptr(s, n_samp) > csc_ptr(s, 0)) {
    if (!s.values) return fail(c, ICIKT_E_INVALID, w + ": X->values is null (the matrix has entries)");
    if (!s.indices) return fail(c, ICIKT_E_INVALID, w + ": X->indices is null (the matrix has entries)");
  }
  return ICIKT_SUCCESS;
}

}  // namespace host
}  // namespace icikt

using icikt::host::check_shape;
using icikt::host::check_view;
using icikt::host::f64_view;

static int check_col_range(icikt_ctx* c, int64_t n_samp, int64_t col_begin, int64_t col_end, int64_t alloc_cols,
                           int64_t n_feat = 0) {
  if (n_feat > ICIKT_MAX_FEATURES && (col_begin != 0 || col_end != n_samp))   // the sharded pre-pass exchanges 16-bit arrays
    return fail(c, ICIKT_E_TOO_LONG, std::string("prepare (column range): ") + kNoWide);
  if (col_begin < 0 || col_end < col_begin || col_end > n_samp || alloc_cols < n_samp)
    return fail(c, ICIKT_E_INVALID, "prepare: bad column range");
  // rec is interleaved in blocks of two columns: a column range is contiguous memory only on even boundaries
  // (an EMPTY range is fine wherever it sits: a rank beyond the last column of an odd-width matrix has [n_samp, n_samp))
  if (col_begin < col_end && ((col_begin & 1) || ((col_end & 1) && col_end != n_samp)))
    return fail(c, ICIKT_E_INVALID, "prepare: a column range must start on an even column and end on one (or at n_samp)");
  return ICIKT_SUCCESS;
}

using icikt::host::prepare_alloc;
using icikt::host::prepare_launch;

static int prepare_impl(icikt_ctx* c, const double* dX, int64_t n_feat, int64_t n_samp, int64_t ld,
                        int64_t col_begin, int64_t col_end, int64_t alloc_cols, uint32_t flags) {
  if (!c) return ICIKT_E_INVALID;
  int rc = check_shape(c, "prepare", n_feat, n_samp, ld);
  if (rc) return rc;
  if (n_samp > 0 && n_feat > 0 && !dX) return fail(c, ICIKT_E_INVALID, "prepare: null matrix");
  rc = check_col_range(c, n_samp, col_begin, col_end, alloc_cols, n_feat);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  rc = prepare_alloc(c, n_feat, n_samp, alloc_cols, col_end - col_begin);
  if (rc) return rc;
  rc = timer_begin(c, ICIKT_K_PREPARE, flags);
  if (rc) return rc;
  rc = prepare_launch(c, dX, ld, col_begin, col_end);
  if (rc) return rc;
  rc = timer_end(c, ICIKT_K_PREPARE, flags);
  if (rc) return rc;
  c->prepared = true;
  return ICIKT_SUCCESS;
}

extern "C" {

int icikt_prepare_dev(icikt_ctx* c, const double* dX, int64_t n_feat, int64_t n_samp, int64_t ld, uint32_t flags) {
  return prepare_impl(c, dX, n_feat, n_samp, ld, 0, n_samp, n_samp, flags);
}

int icikt_prepare_cols_dev(icikt_ctx* c, const double* dX, int64_t n_feat, int64_t n_samp, int64_t ld,
                           int64_t col_begin, int64_t col_end, int64_t alloc_cols, uint32_t flags) {
  return prepare_impl(c, dX, n_feat, n_samp, ld, col_begin, col_end, alloc_cols, flags);
}

int icikt_prepare_cols_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                           int64_t col_begin, int64_t col_end, int64_t alloc_cols, uint32_t flags) {
  if (!c) return ICIKT_E_INVALID;
  int rc = check_shape(c, "prepare", n_feat, n_samp, ld);
  if (rc) return rc;
  if (n_samp > 0 && n_feat > 0 && !X) return fail(c, ICIKT_E_INVALID, "prepare: null matrix");
  rc = check_col_range(c, n_samp, col_begin, col_end, alloc_cols, n_feat);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  rc = prepare_alloc(c, n_feat, n_samp, alloc_cols, col_end - col_begin);
  if (rc) return rc;
  const icikt::host::PinnedScope scope(c, flags);
  rc = icikt::host::upload_and_prepare(c, f64_view(X, ld), n_feat, n_samp, col_begin, col_end, flags);
  if (rc) return rc;
  c->prepared = true;
  return ICIKT_SUCCESS;
}

int icikt_expand_cols_dev(icikt_ctx* c, int64_t col_begin, int64_t col_end, uint32_t flags) {
  if (!c) return ICIKT_E_INVALID;
  if (!c->prepared) return fail(c, ICIKT_E_STATE, "expand_cols: nothing prepared");
  if (col_begin < 0 || col_end < col_begin || col_end > c->pv.n_samp)
    return fail(c, ICIKT_E_INVALID, "expand_cols: bad column range");
  if (c->pv.wide) return fail(c, ICIKT_E_TOO_LONG, std::string("expand_cols: ") + kNoWide);
  int rc = use_device(c);
  if (rc) return rc;
  c->raw_valid = false;
  rc = timer_begin(c, ICIKT_K_PREPARE, flags);
  if (rc) return rc;
  HIPCHK(c, icikt::launch_k0_expand(c->pv, (int)col_begin, (int)(col_end - col_begin), c->stream));
  return timer_end(c, ICIKT_K_PREPARE, flags);
}

int icikt_prep_arrays(icikt_ctx* c, void** ptrs, int64_t* bytes_per_col) {
  if (!c || !ptrs || !bytes_per_col) return ICIKT_E_INVALID;
  if (!c->prepared) return fail(c, ICIKT_E_STATE, "prep_arrays: nothing prepared");
  if (c->pv.wide) return fail(c, ICIKT_E_TOO_LONG, std::string("prep_arrays: ") + kNoWide);
  const PrepView& pv = c->pv;
  ptrs[0] = pv.order;    bytes_per_col[0] = (int64_t)pv.n_ord * 2;
  ptrs[1] = pv.rec;      bytes_per_col[1] = (int64_t)pv.rec_rows * 4;
  ptrs[2] = pv.hirow;    bytes_per_col[2] = (int64_t)pv.rec_rows * 2;
  ptrs[3] = pv.meta;     bytes_per_col[3] = (int64_t)pv.mstride * 8;
  ptrs[4] = pv.tgroups;  bytes_per_col[4] = (int64_t)pv.tg_stride * 4;
  return ICIKT_SUCCESS;
}

int icikt_set_pairs(icikt_ctx* c, const int32_t* pi, const int32_t* pj, int64_t n_pairs) {
  if (!c) return ICIKT_E_INVALID;
  if (n_pairs < 0 || (n_pairs > 0 && (!pi || !pj))) return fail(c, ICIKT_E_INVALID, "set_pairs: bad pair list");
  if (n_pairs >= ((int64_t)1 << 31) - 1) return fail(c, ICIKT_E_INVALID, "set_pairs: more than 2^31-2 pairs");
  int rc = use_device(c);
  if (rc) return rc;
  int32_t mx = -1;
  for (int64_t p = 0; p < n_pairs; ++p) {
    if (pi[p] < 0 || pj[p] < 0) return fail(c, ICIKT_E_INVALID, "set_pairs: negative column index");
    mx = std::max(mx, std::max(pi[p], pj[p]));
  }
  try {
    c->h_pi.assign(pi, pi + n_pairs);
    c->h_pj.assign(pj, pj + n_pairs);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "set_pairs: host allocation failed");
  }
  c->n_pairs = n_pairs;
  c->pairs_nsamp = (int64_t)mx + 1;
  c->raw_valid = false;
  c->wpb = 0;  // units are (re)built at run time for the plan of the prepared matrix
  c->combn_S = -1;
  c->h_pairs_valid = true;
  return icikt::host::upload_pairs(c);
}

int icikt_set_pairs_combn(icikt_ctx* c, int64_t n_samp, int64_t begin, int64_t end) {
  if (!c) return ICIKT_E_INVALID;
  const int64_t total = n_samp * (n_samp - 1) / 2;
  if (n_samp < 0 || begin < 0 || end < begin || end > total)
    return fail(c, ICIKT_E_INVALID, "set_pairs_combn: range outside C(n_samp, 2)");
  if (end - begin >= ((int64_t)1 << 31) - 1) return fail(c, ICIKT_E_INVALID, "set_pairs_combn: too many pairs");
  int rc = use_device(c);
  if (rc) return rc;
  // the pair arrays of a combn range are arithmetic: a kernel fills the device copies (no host loop, no upload);
  // the host copies are made only if a host-built task list needs them (ensure_host_pairs)
  c->n_pairs = end - begin;
  c->pairs_nsamp = n_samp;
  c->raw_valid = false;
  c->wpb = 0;
  c->combn_S = n_samp; c->combn_begin = begin; c->combn_end = end;
  c->h_pairs_valid = false;
  const int64_t P = c->n_pairs;
  HIPCHK(c, c->d_pi.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, c->d_pj.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, c->d_raw.reserve((size_t)std::max<int64_t>(P, 1)));
  HIPCHK(c, icikt::launch_fill_combn(c->d_pi.p, c->d_pj.p, n_samp, begin, P, c->stream));
  return ICIKT_SUCCESS;
}

int64_t icikt_num_pairs(const icikt_ctx* c) { return c ? c->n_pairs : -1; }

int icikt_run_dev(icikt_ctx* c, int perspective, int alternative, int continuity, uint32_t flags,
                  double* d_out4, int64_t* d_counts, int32_t* d_reasons) {
  if (!c) return ICIKT_E_INVALID;
  if (!c->prepared) return fail(c, ICIKT_E_STATE, "run: icikt_prepare_dev has not been called");
  if (c->n_pairs < 0) return fail(c, ICIKT_E_STATE, "run: no pair list set");
  if (perspective != ICIKT_PERSPECTIVE_LOCAL && perspective != ICIKT_PERSPECTIVE_GLOBAL)
    return fail(c, ICIKT_E_INVALID, "run: perspective must be local (0) or global (1)");
  if (alternative < 0 || alternative > ICIKT_ALT_OTHER) return fail(c, ICIKT_E_INVALID, "run: bad alternative code");
  if (c->pairs_nsamp > c->pv.n_samp) return fail(c, ICIKT_E_INVALID, "run: pair list refers to a column >= n_samp");
  if (c->n_pairs > 0 && !d_out4) return fail(c, ICIKT_E_INVALID, "run: null output");
  int rc = use_device(c);
  if (rc) return rc;
  if (c->n_pairs == 0) return ICIKT_SUCCESS;

  // The pair kernel's counts (dis, joint ties, both-missing rows) do not depend on perspective, alternative or
  // continuity: with ICIKT_FLAG_REUSE_COUNTS a second run over the same prepared matrix and pair list (the other
  // perspective of BASELINE config 5, another alternative) is the epilogue alone.
  const bool reuse = (flags & ICIKT_FLAG_REUSE_COUNTS) && c->raw_valid;
  if (c->pv.n > 0 && !reuse) {
    rc = icikt::host::run_counts(c, flags);
    if (rc) return rc;
  }
  // (wide columns: exact integer arithmetic in the epilogue)
  const int exact64 = (c->pv.wide || (flags & ICIKT_FLAG_EXACT_INT64)) ? 1 : 0;
  rc = timer_begin(c, ICIKT_K_EPILOGUE, flags);
  if (rc) return rc;
  HIPCHK(c, icikt::launch_k2(c->pv, c->d_pi.p, c->d_pj.p, c->d_raw.p, c->n_pairs, perspective, alternative,
                             continuity ? 1 : 0, exact64, d_out4, d_counts, d_reasons, c->stream));
  return timer_end(c, ICIKT_K_EPILOGUE, flags);
}

int icikt_kernel_ms(icikt_ctx* c, int kernel, double* ms, int64_t* launches) {
  if (!c || kernel < 0 || kernel >= ICIKT_K_COUNT) return ICIKT_E_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  rc = flush_timer(c, kernel);
  if (rc) return rc;
  if (ms) *ms = c->ms[kernel];
  if (launches) *launches = c->launches[kernel];
  return ICIKT_SUCCESS;
}

int icikt_reset_timers(icikt_ctx* c) {
  if (!c) return ICIKT_E_INVALID;
  for (int k = 0; k < ICIKT_K_COUNT; ++k) {
    int rc = flush_timer(c, k);
    if (rc) return rc;
    c->ms[k] = 0.0;
    c->launches[k] = 0;
  }
  return ICIKT_SUCCESS;
}

}  // extern "C"

namespace icikt {
namespace host {

// every index of a host pair list inside [0, n_samp)
int check_pair_list(icikt_ctx* c, const char* who, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int64_t n_samp) {
  if (n_pairs < 0 || (n_pairs > 0 && (!pi || !pj))) return fail(c, ICIKT_E_INVALID, std::string(who) + ": bad pair list");
  for (int64_t p = 0; p < n_pairs; ++p)
    if (pi[p] < 0 || pi[p] >= n_samp || pj[p] < 0 || pj[p] >= n_samp)
      return fail(c, ICIKT_E_INVALID, std::string(who) + ": column index out of range");
  return ICIKT_SUCCESS;
}

int check_pair_args(icikt_ctx* c, const char* who, const MatrixSrc& X, int64_t n_feat, int64_t n_samp,
                    const int32_t* pi, const int32_t* pj, int64_t* n_pairs, const void* out, bool out5,
                    int perspective, int alternative) {
  const std::string w(who);
  int rc = check_src(c, who, X, n_feat, n_samp);
  if (rc) return rc;
  if (pi == nullptr) {
    if (pj != nullptr) return fail(c, ICIKT_E_INVALID, w + ": pi is null but pj is not");
    *n_pairs = n_samp * (n_samp - 1) / 2;
  } else {
    rc = check_pair_list(c, who, pi, pj, *n_pairs, n_samp);
    if (rc) return rc;
  }
  if ((out5 ? n_samp : *n_pairs) > 0 && !out) return fail(c, ICIKT_E_INVALID, w + ": null output");
  if (perspective != ICIKT_PERSPECTIVE_LOCAL && perspective != ICIKT_PERSPECTIVE_GLOBAL)
    return fail(c, ICIKT_E_INVALID, w + ": perspective must be local (0) or global (1)");
  if (alternative < 0 || alternative > ICIKT_ALT_OTHER) return fail(c, ICIKT_E_INVALID, w + ": bad alternative code");
  return ICIKT_SUCCESS;
}

}  // namespace host
}  // namespace icikt
using icikt::host::check_pair_list;
using icikt::host::MatrixSrc;

static int pairs_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                     const int32_t* pj, int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                     double* out4, int64_t* counts, int32_t* reasons);
static int matrix_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                      int n_global_na, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int perspective,
                      int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double* out5,
                      uint8_t* keep, int64_t* reason_counts);

extern "C" {

int icikt_pairs_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                    const int32_t* pi, const int32_t* pj, int64_t n_pairs, int perspective, int alternative,
                    int continuity, uint32_t flags, double* out4, int64_t* counts, int32_t* reasons) {
  const icikt_input v = f64_view(X, ld);
  return icikt_pairs_in(c, &v, n_feat, n_samp, pi, pj, n_pairs, perspective, alternative, continuity, flags, out4, counts,
                        reasons);
}

int icikt_pairs_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                   const int32_t* pj, int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                   double* out4, int64_t* counts, int32_t* reasons) {
  return pairs_src(c, MatrixSrc::dense(X), n_feat, n_samp, pi, pj, n_pairs, perspective, alternative, continuity, flags, out4,
                   counts, reasons);
}

int icikt_pairs_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                    const int32_t* pj, int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                    double* out4, int64_t* counts, int32_t* reasons) {
  return pairs_src(c, MatrixSrc::csc(X), n_feat, n_samp, pi, pj, n_pairs, perspective, alternative, continuity, flags, out4,
                   counts, reasons);
}

}  // extern "C"

// the body of icikt_pairs_in / icikt_pairs_csc
static int pairs_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                     const int32_t* pj, int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                     double* out4, int64_t* counts, int32_t* reasons) {
  if (!c) return ICIKT_E_INVALID;
  // every argument is validated before the first asynchronous copy reads the caller's memory
  int rc = icikt::host::check_pair_args(c, "pairs", X, n_feat, n_samp, pi, pj, &n_pairs, out4, false, perspective,
                                        alternative);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  rc = pi ? icikt_set_pairs(c, pi, pj, n_pairs) : icikt_set_pairs_combn(c, n_samp, 0, n_pairs);
  if (rc) return rc;
  rc = prepare_alloc(c, n_feat, n_samp, n_samp, n_samp);
  if (rc) return rc;
  // The copies and the pre-pass are only ENQUEUED here; the host builds the pair kernel's task list while the matrix
  // crosses PCIe (it used to wait for the copies first and build the list afterwards, with the GPU idle: 1.2 ms of
  // 14.3 on c4).  Nothing may still read the caller's matrix when the call returns: end_call.
  const icikt::host::PinnedScope scope(c, flags);
  rc = icikt::host::upload_prepare_pairs(c, X, n_feat, n_samp, flags);
  const int64_t P = c->n_pairs;
  if (rc || P == 0) return icikt::host::end_call(c, "pairs", rc);
  auto body = [&]() -> int {
    HIPCHK(c, c->d_out4.reserve((size_t)P * 4));
    if (counts) HIPCHK(c, c->d_counts.reserve((size_t)P * ICIKT_CNT_FIELDS));
    if (reasons) HIPCHK(c, c->d_reasons.reserve((size_t)P));
    // (pipelined: the pair kernel has been enqueued chunk by chunk already -- raw_valid -- and this is the epilogue alone)
    int r = icikt_run_dev(c, perspective, alternative, continuity, flags | (c->raw_valid ? ICIKT_FLAG_REUSE_COUNTS : 0u),
                          c->d_out4.p, counts ? c->d_counts.p : nullptr, reasons ? c->d_reasons.p : nullptr);
    if (r) return r;
    r = icikt::host::download(c, out4, c->d_out4.p, (size_t)P * 4 * sizeof(double));
    if (!r && counts) r = icikt::host::download(c, counts, c->d_counts.p, (size_t)P * ICIKT_CNT_FIELDS * sizeof(int64_t));
    if (!r && reasons) r = icikt::host::download(c, reasons, c->d_reasons.p, (size_t)P * sizeof(int32_t));
    return r;
  };
  // success or not: nothing may still be reading or writing the caller's buffers when this returns
  return icikt::host::end_call(c, "pairs", body());
}

namespace icikt {
namespace host {

// global_na (R/utils.R:1-23) -> the pre-pass's exclusion rule
int make_mask_spec(icikt_ctx* c, const double* global_na, int n_global_na, icikt::MaskSpec* ms) {
  *ms = icikt::MaskSpec{};
  if (n_global_na < 0 || (n_global_na > 0 && !global_na)) return fail(c, ICIKT_E_INVALID, "matrix: bad global_na");
  for (int k = 0; k < n_global_na; ++k) {
    const double v = global_na[k];
    if (v != v) ms->mask_nan = 1;
    else if (v - v != 0.0) ms->mask_inf = 1;   // +-Inf
    else {
      bool dup = false;
      for (int q = 0; q < ms->n_vals; ++q) dup = dup || ms->vals[q] == v;
      if (dup) continue;
      if (ms->n_vals == icikt::ICIKT_MASK_VALS)
        return fail(c, ICIKT_E_INVALID, "matrix: more than 32 distinct finite values in global_na (mask the matrix on the host and pass NaN)");
      ms->vals[ms->n_vals++] = v;
    }
  }
  return ICIKT_SUCCESS;
}

}  // namespace host
}  // namespace icikt

extern "C" {

// ici_kendalltau() below the argument checks, in one call: exclusion rule + pre-pass + pair kernel + epilogue +
// scale_and_reshape on the device, one D2H of the five matrices.
int icikt_matrix_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld, const double* global_na,
                     int n_global_na, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int perspective,
                     int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double* out5,
                     uint8_t* keep, int64_t* reason_counts) {
  const icikt_input v = f64_view(X, ld);
  return icikt_matrix_in(c, &v, n_feat, n_samp, global_na, n_global_na, pi, pj, n_pairs, perspective, alternative,
                         continuity, flags, scale_max, diag_good, out5, keep, reason_counts);
}

int icikt_matrix_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                    int n_global_na, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int perspective,
                    int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double* out5,
                    uint8_t* keep, int64_t* reason_counts) {
  return matrix_src(c, MatrixSrc::dense(X), n_feat, n_samp, global_na, n_global_na, pi, pj, n_pairs, perspective, alternative,
                    continuity, flags, scale_max, diag_good, out5, keep, reason_counts);
}

int icikt_matrix_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const double* global_na,
                     int n_global_na, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int perspective,
                     int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double* out5,
                     uint8_t* keep, int64_t* reason_counts) {
  return matrix_src(c, MatrixSrc::csc(X), n_feat, n_samp, global_na, n_global_na, pi, pj, n_pairs, perspective, alternative,
                    continuity, flags, scale_max, diag_good, out5, keep, reason_counts);
}

}  // extern "C"

// the body of icikt_matrix_in / icikt_matrix_csc
static int matrix_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const double* global_na,
                      int n_global_na, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int perspective,
                      int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double* out5,
                      uint8_t* keep, int64_t* reason_counts) {
  if (!c) return ICIKT_E_INVALID;
  int rc = icikt::host::check_pair_args(c, "matrix", X, n_feat, n_samp, pi, pj, &n_pairs, out5, true, perspective,
                                        alternative);
  if (rc) return rc;
  icikt::MaskSpec ms;
  rc = icikt::host::make_mask_spec(c, global_na, n_global_na, &ms);
  if (rc) return rc;
  if (reason_counts) for (int k = 0; k < 5; ++k) reason_counts[k] = 0;
  if (n_samp == 0) return ICIKT_SUCCESS;
  rc = use_device(c);
  if (rc) return rc;
  rc = pi ? icikt_set_pairs(c, pi, pj, n_pairs) : icikt_set_pairs_combn(c, n_samp, 0, n_pairs);
  if (rc) return rc;
  rc = prepare_alloc(c, n_feat, n_samp, n_samp, n_samp);
  if (rc) return rc;
  const size_t S = (size_t)n_samp, P = (size_t)c->n_pairs;
  const size_t keep_bytes = keep ? S * (size_t)n_feat : 0;
  if (keep_bytes) HIPCHK(c, c->d_keep.reserve(keep_bytes));
  HIPCHK(c, c->d_out5.reserve(5 * S * S));
  HIPCHK(c, c->d_red.reserve(8));
  HIPCHK(c, c->d_out4.reserve(std::max<size_t>(P, 1) * 4));
  HIPCHK(c, c->d_reasons.reserve(std::max<size_t>(P, 1)));
  const icikt::host::PinnedScope scope(c, flags);
  c->k0_mask = &ms;
  c->k0_keep = keep_bytes ? c->d_keep.p : nullptr;
  rc = icikt::host::upload_prepare_pairs(c, X, n_feat, n_samp, flags);
  c->k0_mask = nullptr;
  c->k0_keep = nullptr;
  if (rc) return icikt::host::end_call(c, "matrix", rc);
  unsigned long long red[8] = {};
  auto body = [&]() -> int {
    int r = icikt_run_dev(c, perspective, alternative, continuity, flags | (c->raw_valid ? ICIKT_FLAG_REUSE_COUNTS : 0u),
                          c->d_out4.p, nullptr, c->d_reasons.p);
    if (r) return r;
    HIPCHK(c, icikt::launch_out_stats(c->pv, c->d_out4.p, c->d_reasons.p, (int64_t)P, nullptr, c->d_red.p, c->stream));
    HIPCHK(c, icikt::launch_assemble(c->pv, c->d_out4.p, c->d_pi.p, c->d_pj.p, (int64_t)P, nullptr, c->d_red.p,
                                     scale_max ? 1 : 0, diag_good ? 1 : 0, c->d_out5.p, c->stream));
    r = icikt::host::download(c, out5, c->d_out5.p, 5 * S * S * sizeof(double));
    if (!r && keep_bytes) r = icikt::host::download(c, keep, c->d_keep.p, keep_bytes);
    if (!r) r = icikt::host::download(c, red, c->d_red.p, sizeof(red));
    return r;
  };
  rc = icikt::host::end_call(c, "matrix", body());
  if (rc) return rc;
  if (reason_counts) for (int k = 0; k < 5; ++k) reason_counts[k] = (int64_t)red[1 + k];
  return ICIKT_SUCCESS;
}

extern "C" {

// kt_fast(use = "pairwise.complete.obs"): every pair gets its own two columns with the rows that miss either value
// masked in both (k_mask_pairs), sorted (K0) and counted (K1, one pair per wave) on the device; the perspective is
// "local" by construction.  Pairs go through in chunks that keep the masked columns within ~1.5 GiB.
int icikt_pairs_complete_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                             const int32_t* pi, const int32_t* pj, int64_t n_pairs, int alternative, int continuity,
                             uint32_t flags, double* out4, int64_t* counts, int32_t* reasons) {
  const icikt_input v = f64_view(X, ld);
  return icikt_pairs_complete_in(c, &v, n_feat, n_samp, pi, pj, n_pairs, alternative, continuity, flags, out4, counts,
                                 reasons);
}

int icikt_pairs_complete_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                            const int32_t* pj, int64_t n_pairs, int alternative, int continuity, uint32_t flags,
                            double* out4, int64_t* counts, int32_t* reasons) {
  if (!c) return ICIKT_E_INVALID;
  int rc = check_view(c, "pairs_complete", X, n_feat, n_samp, /*wide_ok=*/false);
  if (rc) return rc;
  rc = check_pair_list(c, "pairs_complete", pi, pj, n_pairs, n_samp);
  if (rc) return rc;
  if (n_pairs == 0) return ICIKT_SUCCESS;
  if (!out4) return fail(c, ICIKT_E_INVALID, "pairs_complete: null output");
  if (alternative < 0 || alternative > ICIKT_ALT_OTHER) return fail(c, ICIKT_E_INVALID, "pairs_complete: bad alternative code");
  rc = use_device(c);
  if (rc) return rc;
  // the matrix and the pair list, once
  rc = icikt_set_pairs(c, pi, pj, n_pairs);
  if (rc) return rc;
  const icikt::host::PinnedScope scope(c, flags);
  DevBuf<int32_t> all_pi, all_pj;  // the caller's list stays on the device while d_pi / d_pj hold a chunk's (2k, 2k+1)
  HIPCHK(c, all_pi.reserve((size_t)n_pairs));
  HIPCHK(c, all_pj.reserve((size_t)n_pairs));
  auto body = [&]() -> int {
    HIPCHK(c, hipMemcpyAsync(all_pi.p, c->d_pi.p, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(all_pj.p, c->d_pj.p, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    int r = ICIKT_SUCCESS;
    if (n_feat > 0) {  // H2D of the matrix (staged like every other matrix upload); none of its own columns is sorted, only the masked pair columns are
      r = icikt::host::upload_and_prepare(c, *X, n_feat, n_samp, 0, n_samp, 0u, false, nullptr, icikt::host::kPrepassNone);
      if (r) return r;
    }
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_pairs, ((int64_t)3 << 29) / std::max<int64_t>(16 * n_feat, 16)));
    HIPCHK(c, c->d_Xp.reserve((size_t)std::max<int64_t>(2 * chunk * n_feat, 1)));
    HIPCHK(c, c->d_out4.reserve((size_t)chunk * 4));
    if (counts) HIPCHK(c, c->d_counts.reserve((size_t)chunk * ICIKT_CNT_FIELDS));
    if (reasons) HIPCHK(c, c->d_reasons.reserve((size_t)chunk));
    std::vector<int32_t> qi, qj;
    for (int64_t first = 0; first < n_pairs; first += chunk) {
      const int64_t m = std::min(chunk, n_pairs - first);
      HIPCHK(c, icikt::launch_mask_pairs(c->d_X.p, n_feat, (int)n_feat, all_pi.p, all_pj.p, first, m, c->d_Xp.p, c->stream));
      r = icikt_prepare_dev(c, c->d_Xp.p, n_feat, 2 * m, n_feat, flags);
      if (r) return r;
      if ((int64_t)qi.size() != m) {
        qi.resize((size_t)m); qj.resize((size_t)m);
        for (int64_t k = 0; k < m; ++k) { qi[(size_t)k] = (int32_t)(2 * k); qj[(size_t)k] = (int32_t)(2 * k + 1); }
        r = icikt_set_pairs(c, qi.data(), qj.data(), m);
        if (r) return r;
      }
      r = icikt_run_dev(c, ICIKT_PERSPECTIVE_LOCAL, alternative, continuity, flags, c->d_out4.p,
                        counts ? c->d_counts.p : nullptr, reasons ? c->d_reasons.p : nullptr);
      if (r) return r;
      r = icikt::host::download(c, out4 + 4 * first, c->d_out4.p, (size_t)m * 4 * sizeof(double));
      if (!r && counts) r = icikt::host::download(c, counts + ICIKT_CNT_FIELDS * first, c->d_counts.p, (size_t)m * ICIKT_CNT_FIELDS * sizeof(int64_t));
      if (!r && reasons) r = icikt::host::download(c, reasons + first, c->d_reasons.p, (size_t)m * sizeof(int32_t));
      if (r) return r;
      HIPCHK(c, icikt::host::finish_stream(c, true));   // the chunk's buffers are reused by the next one
    }
    return ICIKT_SUCCESS;
  };
  const int rb = body();
  // the prepared matrix and the pair list are the last chunk's scratch columns and its (2k, 2k+1): nothing of the caller's.
  // The device-resident calls start over (icikt_run_dev: ICIKT_E_STATE until icikt_prepare_dev and a pair list)
  icikt::host::forget_prepared(c);
  return icikt::host::end_call(c, "pairs_complete", rb);
}

int icikt_pair_f64(icikt_ctx* c, const double* x, const double* y, int64_t n, int perspective, int alternative,
                   int continuity, uint32_t flags, double* out4, int64_t* counts, int32_t* reason) {
  if (!c) return ICIKT_E_INVALID;
  if (n < 0 || (n > 0 && (!x || !y))) return fail(c, ICIKT_E_INVALID, "pair: bad vectors");
  if (n > ICIKT_MAX_FEATURES_WIDE) return fail(c, ICIKT_E_TOO_LONG, std::string("pair: ") + kTooLong);
  std::vector<double> xy;
  try {
    xy.resize((size_t)std::max<int64_t>(2 * n, 1));
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "pair: host allocation failed");
  }
  if (n > 0) {
    memcpy(xy.data(), x, (size_t)n * sizeof(double));
    memcpy(xy.data() + n, y, (size_t)n * sizeof(double));
  }
  const int32_t pi = 0, pj = 1;
  // (the two vectors travel in a vector of this function's: whatever the caller says about ITS memory does not hold for it)
  return icikt_pairs_f64(c, xy.data(), n, 2, n, &pi, &pj, 1, perspective, alternative, continuity,
                         flags & ~ICIKT_FLAG_HOST_PINNED, out4, counts, reason);
}

int icikt_missingness_f64(icikt_ctx* c, const double* X, int64_t n_feat, int64_t n_samp, int64_t ld,
                          const int32_t* pi, const int32_t* pj, int64_t n_pairs, int64_t* missingness) {
  const icikt_input v = f64_view(X, ld);
  return icikt_missingness_in(c, &v, n_feat, n_samp, pi, pj, n_pairs, missingness);
}

// the body of icikt_missingness_in / icikt_missingness_csc
static int missingness_src(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                           const int32_t* pj, int64_t n_pairs, int64_t* missingness) {
  if (!c) return ICIKT_E_INVALID;
  int rc = icikt::host::check_src(c, "missingness", X, n_feat, n_samp);
  if (rc) return rc;
  if (n_pairs < 0) return fail(c, ICIKT_E_INVALID, "missingness: bad shape");
  if (n_pairs == 0) return ICIKT_SUCCESS;
  if (!pi || !pj || !missingness) return fail(c, ICIKT_E_INVALID, "missingness: null argument");
  rc = check_pair_list(c, "missingness", pi, pj, n_pairs, n_samp);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  rc = icikt_set_pairs(c, pi, pj, n_pairs);
  if (rc) return rc;
  // The mask-only pre-pass (k0_mask): one streaming pass over each column chunk as it arrives, no sort -- the
  // reference's missing_either (R/kendalltau.R:626-629) is sum(in_x | in_y) and nothing more.
  rc = icikt::host::mask_alloc(c, n_feat, n_samp);
  if (rc) return rc;
  if (n_feat > 0) {
    rc = icikt::host::upload_and_prepare(c, X, n_feat, n_samp, 0, n_samp, 0u, false, nullptr, icikt::host::kPrepassMask);
    if (rc) return rc;
  }
  auto body = [&]() -> int {
    HIPCHK(c, c->d_counts.reserve((size_t)n_pairs));
    HIPCHK(c, icikt::launch_missingness(c->pv, c->d_pi.p, c->d_pj.p, n_pairs, c->d_counts.p, c->stream));
    return icikt::host::download(c, missingness, c->d_counts.p, (size_t)n_pairs * sizeof(int64_t));
  };
  return icikt::host::end_call(c, "missingness", body());
}

int icikt_missingness_in(icikt_ctx* c, const icikt_input* X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                         const int32_t* pj, int64_t n_pairs, int64_t* missingness) {
  return missingness_src(c, MatrixSrc::dense(X), n_feat, n_samp, pi, pj, n_pairs, missingness);
}

int icikt_missingness_csc(icikt_ctx* c, const icikt_csc_input* X, int64_t n_feat, int64_t n_samp, const int32_t* pi,
                          const int32_t* pj, int64_t n_pairs, int64_t* missingness) {
  return missingness_src(c, MatrixSrc::csc(X), n_feat, n_samp, pi, pj, n_pairs, missingness);
}

int icikt_convert_dev(icikt_ctx* c, const void* d_src, int dtype, int order, int64_t n_feat, int64_t n_samp, int64_t ld,
                      double* d_dst, int64_t dst_ld) {
  if (!c) return ICIKT_E_INVALID;
  const icikt_input v{d_src, dtype, order, ld};
  int rc = check_view(c, "convert", &v, n_feat, n_samp);
  if (rc) return rc;
  if (dst_ld < n_feat) return fail(c, ICIKT_E_INVALID, "convert: dst_ld is below n_feat");
  if (n_feat == 0 || n_samp == 0) return ICIKT_SUCCESS;
  if (!d_dst) return fail(c, ICIKT_E_INVALID, "convert: null d_dst");
  rc = use_device(c);
  if (rc) return rc;
  HIPCHK(c, icikt::launch_ingest(d_src, dtype, order, ld, n_feat, n_samp, d_dst, dst_ld, c->stream));
  return ICIKT_SUCCESS;
}

int icikt_scatter_csc_dev(icikt_ctx* c, const void* d_values, const void* d_indices, const void* d_indptr, int dtype,
                          int index_type, double fill, int64_t n_feat, int64_t n_samp, double* d_dst, int64_t dst_ld) {
  if (!c) return ICIKT_E_INVALID;
  if (dtype < ICIKT_DTYPE_F64 || dtype > ICIKT_DTYPE_I64)
    return fail(c, ICIKT_E_INVALID, "scatter_csc: dtype must be one of ICIKT_DTYPE_F64, _F32, _I32, _I64");
  if (index_type != ICIKT_INDEX_I32 && index_type != ICIKT_INDEX_I64)
    return fail(c, ICIKT_E_INVALID, "scatter_csc: index_type must be ICIKT_INDEX_I32 or ICIKT_INDEX_I64");
  int rc = check_shape(c, "scatter_csc", n_feat, n_samp, n_feat);
  if (rc) return rc;
  if (dst_ld < n_feat) return fail(c, ICIKT_E_INVALID, "scatter_csc: dst_ld is below n_feat");
  if (n_feat == 0 || n_samp == 0) return ICIKT_SUCCESS;
  if (!d_dst) return fail(c, ICIKT_E_INVALID, "scatter_csc: null d_dst");
  if (!d_indptr) return fail(c, ICIKT_E_INVALID, "scatter_csc: null d_indptr");
  rc = use_device(c);
  if (rc) return rc;
  // the column offsets are read back and checked as the host entries check theirs: O(n_samp)
  const size_t is = icikt::host::index_bytes(index_type);
  std::vector<char> hp;
  try {
    hp.resize((size_t)(n_samp + 1) * is);
  } catch (const std::bad_alloc&) {
    return fail(c, ICIKT_E_NOMEM, "scatter_csc: host allocation failed");
  }
  HIPCHK(c, hipMemcpyAsync(hp.data(), d_indptr, hp.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const icikt_csc_input v{d_values, d_indices, hp.data(), dtype, index_type, fill};
  // (values / indices are device pointers: check_src only asks whether they are null)
  rc = icikt::host::check_src(c, "scatter_csc", MatrixSrc::csc(&v), n_feat, n_samp);
  if (rc) return rc;
  const int64_t nnz = icikt::host::csc_ptr(v, n_samp);
  HIPCHK(c, c->d_csc_err.reserve(icikt::ICIKT_CSC_ERR_WORDS));
  HIPCHK(c, hipMemsetAsync(c->d_csc_err.p, 0, icikt::ICIKT_CSC_ERR_WORDS * sizeof(unsigned long long), c->stream));
  HIPCHK(c, icikt::launch_scatter_csc(d_values, dtype, d_indices, d_indptr, index_type, 0, 0, nnz, fill, n_feat, n_samp,
                                      d_dst, dst_ld, c->d_csc_err.p, c->stream));
  unsigned long long rec[icikt::ICIKT_CSC_ERR_WORDS] = {};
  HIPCHK(c, hipMemcpyAsync(rec, c->d_csc_err.p, sizeof(rec), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rec[0] != 0) return fail(c, ICIKT_E_INVALID, "scatter_csc: " + icikt::host::csc_message(rec));
  return ICIKT_SUCCESS;
}

}  // extern "C"

extern "C" {

// Development / test hook: "key=value,key=value" overrides of the pair kernel's launch plan and of the host
// path's H2D mode; NULL or "" restores the library's choices.  Keys: np (pairs per wave: 1 | 2), pend (ignored),
// wpb (waves per workgroup), half (0 | 1), tgmax (list / count mode up to this many tie groups of the gathered column; -1 =
// row mode), list (list mode up to this many, <= 128), solo (0: no SOLO steps), waves (waves per CU the counter tables may
// cost the launch down to), split (1 | 2 | 4 segments per half-wave task), gridmult (persistent grid as a multiple of the resident waves, always), gridcap (persistent
// grid: at most this many workgroups),
// pipe (0 | 1: the host entries' chunk pipeline off / on whenever possible), k0 (0 | 1: the pre-pass always in its
// 1 024-thread / 256-thread shape), tkblock (icikt_topk_* / icikt_edges_* / icikt_class_medians_*: pairs per block of
// whole combn rows, 1 = a row per block, or per slice of several classes' pair list),
// medlds (icikt_class_medians_*: partners up to which the select kernel stages a sample's keys in LDS, 0 .. 4096),
// qbatch (icikt_quantiles_*: targets per batch of the select, 1 .. 32),
// padjtile (icikt_padjust_*, icikt_anosim_*: keys of a wave's tile of the sort, 1 .. 2^30),
// anoperms (icikt_anosim_*: labellings per upload, 1 .. 2^20), anostrip (icikt_anosim_*: columns of a workgroup of the
// permutation kernel, 1 .. 4096), hcgrid (icikt_hclust_*: workgroups of the rescan kernel, 1 .. 256),
// verbose (0 | 1: print the plan to stderr).
// (The keys h2d and regfail of rounds 2-3 are gone with the mode they steered: the library no longer page-locks
// caller memory, icikt_host.h.)
int icikt_debug_set_plan(icikt_ctx* c, const char* spec) {
  if (!c) return ICIKT_E_INVALID;
  icikt_ctx::PlanOverride ov;
  int pipe = -1, k0 = -1;
  std::string sp = spec ? spec : "";
  size_t pos = 0;
  while (pos < sp.size()) {
    size_t end = sp.find(',', pos);
    if (end == std::string::npos) end = sp.size();
    const std::string item = sp.substr(pos, end - pos);
    pos = end + 1;
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    if (eq == std::string::npos) return fail(c, ICIKT_E_INVALID, "debug_set_plan: expected key=value, got '" + item + "'");
    const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
    if (val.empty()) continue;  // "key=" keeps the default
    if (key == "np") ov.np = atoi(val.c_str());
    else if (key == "pend") {}   // (accepted and ignored: no kernel keeps a bitset of open tie groups any more)
    else if (key == "wpb") ov.wpb = atoi(val.c_str());
    else if (key == "half") ov.half = (val[0] == '1') ? 1 : 0;
    else if (key == "hyb") ov.hyb = (val[0] == '1') ? 1 : 0;
    else if (key == "tgmax") { ov.has_tgmax = true; ov.tgmax = atoi(val.c_str()); }
    else if (key == "list") ov.list = atoi(val.c_str());
    else if (key == "solo") ov.solo = atoi(val.c_str());
    else if (key == "split") ov.split = atoi(val.c_str());
    else if (key == "merge") ov.merge = atoi(val.c_str());
    else if (key == "waves") ov.waves = atoi(val.c_str());
    else if (key == "verbose") ov.verbose = (val[0] == '1');
    else if (key == "gridmult") ov.grid_mult = atoi(val.c_str());
    else if (key == "gridcap") ov.grid_cap = atoi(val.c_str());
    else if (key == "pipe") pipe = (val[0] == '1') ? 1 : 0;
    else if (key == "k0") k0 = (val[0] == '1') ? 1 : (val[0] == '2') ? 2 : 0;
    else if (key == "tkblock") ov.tkblock = atoll(val.c_str());
    else if (key == "medlds") {
      ov.medlds = atoi(val.c_str());
      if (ov.medlds < 0 || ov.medlds > icikt::MEDIAN_STAGE_MAX)
        return fail(c, ICIKT_E_INVALID, "debug_set_plan: medlds must be in 0 .. 4096 keys");
    }
    else if (key == "qbatch") {
      ov.qbatch = atoi(val.c_str());
      if (ov.qbatch < 1 || ov.qbatch > icikt::QUANT_BATCH_MAX)
        return fail(c, ICIKT_E_INVALID, "debug_set_plan: qbatch must be in 1 .. 32 targets");
    }
    else if (key == "padjtile") {
      ov.padjtile = atoll(val.c_str());
      if (ov.padjtile < 1 || ov.padjtile > (1ll << 30))
        return fail(c, ICIKT_E_INVALID, "debug_set_plan: padjtile must be in 1 .. 2^30 keys");
    }
    else if (key == "anoperms") {
      ov.anoperms = atoll(val.c_str());
      if (ov.anoperms < 1 || ov.anoperms > icikt::ANO_PERMS_MAX)
        return fail(c, ICIKT_E_INVALID, "debug_set_plan: anoperms must be in 1 .. 2^20 labellings");
    }
    else if (key == "anostrip") {
      ov.anostrip = atoi(val.c_str());
      if (ov.anostrip < icikt::ANO_STRIP_MIN || ov.anostrip > icikt::ANO_STRIP_MAX)
        return fail(c, ICIKT_E_INVALID, "debug_set_plan: anostrip must be in 1 .. 4096 columns");
    }
    else if (key == "hcgrid") {
      ov.hcgrid = atoi(val.c_str());
      if (ov.hcgrid < 1 || ov.hcgrid > icikt::HCLUST_GRID_MAX)
        return fail(c, ICIKT_E_INVALID, "debug_set_plan: hcgrid must be in 1 .. 256 workgroups");
    }
    else return fail(c, ICIKT_E_INVALID, "debug_set_plan: unknown key '" + key + "'");
  }
  c->plan_ov = ov;
  c->pipe_mode = pipe;
  c->k0_shape = k0;

  c->raw_valid = false;
  c->wpb = 0;  // tasks are rebuilt for the new plan
  return ICIKT_SUCCESS;
}

// Development hook: per step kind of the pair kernel [steps x 8 | rows x 8 | wave cycles x 8] since the last reset.
// Only a diagnostic build (-DICIKT_STEP_STATS) counts; the product build answers ICIKT_E_STATE.
int icikt_debug_step_stats(icikt_ctx* c, uint64_t* out24, int reset) {
  if (!c || !out24) return ICIKT_E_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long tmp[24];
  const hipError_t e = icikt::read_step_stats(tmp, reset);
  if (e == hipErrorNotSupported) { (void)hipGetLastError(); return fail(c, ICIKT_E_STATE, "debug_step_stats: not a -DICIKT_STEP_STATS build"); }
  HIPCHK(c, e);
  for (int i = 0; i < 24; ++i) out24[i] = tmp[i];
  return ICIKT_SUCCESS;
}

int icikt_selftest(icikt_ctx* c) {
  if (!c) return ICIKT_E_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(c, c->d_self.reserve(640));
  HIPCHK(c, icikt::launch_selftest(c->d_self.p, c->stream));
  uint32_t h[640];
  HIPCHK(c, hipMemcpyAsync(h, c->d_self.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t l = 0; l < 64; ++l) {
    if (h[l] != (l + 1) * (l + 2) / 2) return fail(c, ICIKT_E_HIP, "selftest: wave_incl_scan mismatch");
    if (h[64 + l] != (l == 0 ? 0xABCDu : 3u * (l - 1))) return fail(c, ICIKT_E_HIP, "selftest: wave_shr1 mismatch");
    if (h[128 + l] != (l < 41 ? 0xFFFFFFFFu : l - 41)) return fail(c, ICIKT_E_HIP, "selftest: repeated wave_shr1 mismatch");
    if (h[256 + l] != (l < 32 ? l : 100u + (l - 32))) return fail(c, ICIKT_E_HIP, "selftest: permlane32_swap[0] mismatch");
    if (h[320 + l] != (l < 32 ? 32u + l : 100u + l)) return fail(c, ICIKT_E_HIP, "selftest: permlane32_swap[1] mismatch");
    const uint32_t k = (l & 31u) + 1, b = (l & 32u) + 1;  // sum of (lane+1) over my half up to me
    if (h[384 + l] != k * (2 * b + k - 1) / 2) return fail(c, ICIKT_E_HIP, "selftest: half_incl_scan mismatch");
    if (h[448 + l] != 63u) {
      if (c->plan_ov.verbose) fprintf(stderr, "[icikt] selftest lane %u: lane_xor pass mask %u\n", l, h[448 + l]);
      return fail(c, ICIKT_E_HIP, "selftest: lane_xor mismatch");
    }
  }
  // half-wave all-pairs: per 32-lane half, #{(a, j): a before j, q_a < lo_j}; the lanes' shares are summed
  for (uint32_t half = 0; half < 2; ++half) {
    uint32_t want = 0, got = 0;
    for (uint32_t l = half * 32; l < half * 32 + 32; ++l) {
      const uint32_t lo = ((l * 40503u + 977u) >> 3) & 0xFFFu;
      for (uint32_t j = half * 32; j < l; ++j) want += (((j * 2654435761u >> 20) & 0xFFFu) < lo) ? 1u : 0u;
      got += h[192 + l];
    }
    if (got != want) {
      if (c->plan_ov.verbose) fprintf(stderr, "[icikt] selftest half %u: got %u want %u\n", half, got, want);
      return fail(c, ICIKT_E_HIP, "selftest: half_allpairs mismatch");
    }
  }
  // ... and the packed form: two sub-steps' rows at once, the counts of both summed
  for (uint32_t half = 0; half < 2; ++half) {
    uint32_t want = 0, got = 0;
    for (uint32_t l = half * 32; l < half * 32 + 32; ++l) {
      const uint32_t lo = ((l * 40503u + 977u) >> 3) & 0xFFFu, lo2 = ((l * 69069u + 12345u) >> 5) & 0x27BFu;
      for (uint32_t j = half * 32; j < l; ++j) {
        want += (((j * 2654435761u >> 20) & 0xFFFu) < lo) ? 1u : 0u;
        want += (((j * 1103515245u >> 17) & 0x27BFu) < lo2) ? 1u : 0u;
      }
      got += h[576 + l];
    }
    if (got != want) {
      if (c->plan_ov.verbose) fprintf(stderr, "[icikt] selftest half %u (packed): got %u want %u\n", half, got, want);
      return fail(c, ICIKT_E_HIP, "selftest: half_step_count mismatch");
    }
  }
  return ICIKT_SUCCESS;
}

}  // extern "C"
