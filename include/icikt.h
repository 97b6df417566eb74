/*
 * icikt.h -- C ABI of the MI355X (gfx950) ICI-Kendall-tau pair engine.
 *
 * This is the drop-in boundary for the reference's hot path
 *   ici_kendalltau() -> ici_split() -> ici_kt()   (R/kendalltau.R:96-308, src/kendallc.cpp:166-366).
 * The reference crosses its FFI once per pair:
 *   .Call('_ICIKendallTau_ici_kt', x, y, perspective, alternative, continuity, output)
 *     R/RcppExports.R:62-64, C symbol SEXP _ICIKendallTau_ici_kt(SEXP x6) src/RcppExports.cpp:83-96
 * This library moves the boundary up to the batch (ici_split, R/kendalltau.R:280-308): one call per
 * pair LIST.  Plain pointers and sizes only; no R, Rcpp or torch types.  The R-side .Call glue a
 * maintainer adds is in icikendalltau_amd/r/ and INTEGRATION.md.
 *
 * Conventions
 *   - X is column-major n_feat x n_samp with leading dimension ld (R matrix layout; columns are
 *     samples, R/kendalltau.R:6).  Missing = NaN of any payload (R's NA_real_ is a NaN;
 *     Rcpp is_na() is true for NA and NaN, src/kendallc.cpp:181).
 *   - The *_in host entries take the same matrix as a typed, strided VIEW (icikt_input): float64, float32, int32 or
 *     int64 cells, column- or row-major, read where it lies.  An entry given a view V returns what its _f64 twin
 *     returns on the column-major float64 matrix M[r, c] = (double)V[r, c]; the widening and the transpose run on
 *     the device (icikt_convert_dev's kernel), never as a host copy.
 *   - Pair indices are 0-based column indices; pair p is ici_kt(x = X[, pi[p]], y = X[, pj[p]]).
 *   - out4 is P x 4 row-major: tau, pvalue, tau_max, completeness (src/kendallc.cpp:171-172).
 *     Degenerate pairs get R's NA_real_ bit pattern (0x7FF00000000007A2) in all four and a reason.
 *   - All functions return ICIKT_SUCCESS (0) or a negative ICIKT_E_* code; the message is kept in
 *     the context (icikt_last_error).  Nothing throws across the boundary.
 *   - n_feat <= ICIKT_MAX_FEATURES (65 535) rows per column run the tuned kernels (16-bit positions).  Longer
 *     columns, up to ICIKT_MAX_FEATURES_WIDE (262 144) rows, are accepted by every single-device entry and run a
 *     plain 32-bit path (about two orders of magnitude slower per pair) in EXACT integer arithmetic: the reference's
 *     int32 wrap-around (its `int dis`, src/kendallc.cpp:78, and the Rcpp-sugar tie sums) is not reproduced there,
 *     i.e. ICIKT_FLAG_EXACT_INT64 is implied.  Beyond that: ICIKT_E_TOO_LONG with a message that names the limit.
 *   - A context owns one HIP device, one stream and its workspaces.  Calls on one context must come
 *     from one thread at a time.  Must not be used in a fork()ed child of a process that has
 *     already created a context (R/utils.R:68-80 furrr multicore workers).
 */
#ifndef ICIKT_H
#define ICIKT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICIKT_VERSION 400 /* 0.4.0: ICIKT_FLAG_HOST_PINNED (no page-locking of caller memory by the library), mask-only missingness pre-pass */

/* status codes */
#define ICIKT_SUCCESS 0
#define ICIKT_E_INVALID (-1)    /* bad argument (message says which) */
#define ICIKT_E_HIP (-2)        /* HIP runtime error */
#define ICIKT_E_NOMEM (-3)      /* host allocation failure */
#define ICIKT_E_TOO_LONG (-4)   /* n_feat > ICIKT_MAX_FEATURES_WIDE (or > ICIKT_MAX_FEATURES where wide columns are not supported) */
#define ICIKT_E_STATE (-5)      /* call order: prepare / set_pairs before run */
#define ICIKT_E_NO_DEVICE (-6)  /* no usable HIP device: the product path never falls back to CPU */

/* n_feat limit of the uint16 rank path.  The reference's `int dis` (src/kendallc.cpp:78) and
 * int32 tie sums are themselves only safe to n ~ 65 535. */
#define ICIKT_MAX_FEATURES 65535
#define ICIKT_MAX_FEATURES_WIDE 262144

/* perspective (src/kendallc.cpp:180) */
#define ICIKT_PERSPECTIVE_LOCAL 0
#define ICIKT_PERSPECTIVE_GLOBAL 1
/* alternative (src/kendallc.cpp:323-332); OTHER = any unrecognised string: p-value stays 0 */
#define ICIKT_ALT_TWO_SIDED 0
#define ICIKT_ALT_LESS 1
#define ICIKT_ALT_GREATER 2
#define ICIKT_ALT_OTHER 3

/* flags */
#define ICIKT_FLAG_EXACT_INT64 1u /* tie sums in int64 instead of the reference's wrapping int32
                                     (count_rank_tie, src/kendallc.cpp:112-114) */
#define ICIKT_FLAG_TIMING 2u      /* record HIP events around each kernel (icikt_kernel_ms) */
#define ICIKT_FLAG_REUSE_COUNTS 4u /* icikt_run_dev: if the pair kernel already ran for this prepared matrix and pair
                                     list, keep its integer counts and run the epilogue only -- "local" is derived
                                     from the same counts as "global", so the second perspective (or another
                                     alternative / continuity) costs microseconds */

#define ICIKT_FLAG_HOST_PINNED 8u  /* host entries: the caller states that the matrix and the result arrays of this call
                                     lie in memory it has page-locked itself (hipHostMalloc / hipHostRegister); they are
                                     then copied from and into directly.  Without it (default) every transfer of 256 KB
                                     or more crosses the library's own pinned buffers: the library never page-locks
                                     and never probes caller memory.  Setting it for pageable memory is a caller error
                                     with the consequences of an asynchronous copy from pageable memory. */

#define ICIKT_FLAG_BALANCE_COST 16u /* icikt_pairs_multi_f64 / icikt_matrix_multi_f64: cut the pair list into blocks of equal COST
                                     instead of equal length.  The reference's chunks are ceiling(n_todo / ncore) pairs each
                                     (R/kendalltau.R:250-255), and one ici_kt costs the same whatever the data; here a pair's
                                     cost follows the tie structure of the column it streams (up to 2.5x between columns), and
                                     the pre-pass leaves that cost with every column.  Blocks stay consecutive in list order
                                     (no block longer than twice the equal share); results are the same, in the same order. */

/* per-pair reason codes; the host wrapper raises the reference's warnings from them */
#define ICIKT_OK 0
#define ICIKT_NA_ALL_MISSING 1   /* src/kendallc.cpp:190-199: silent NA x4 */
#define ICIKT_NA_SHORT 2         /* :224-231 "The vectors only have a single value, NA returned!" */
#define ICIKT_NA_SINGLE_UNIQUE 3 /* :234-244 "Either 'X' or 'Y' have only a single unique value, NA returned!" */
#define ICIKT_NA_TIES_EQ_TOTAL 4 /* :291-298 "Ties equal the total, NA returned!" */

/* int64 counts record per pair (the integers src/kendallc.cpp:342-363 prints when output != "simple") */
#define ICIKT_CNT_N 0        /* n_entry after the perspective's row filter */
#define ICIKT_CNT_MISSING 1  /* rows with x or y missing (:208-211) */
#define ICIKT_CNT_DIS 2      /* kendall_discordant (:69-100) */
#define ICIKT_CNT_NTIE 3     /* joint ties (:267) */
#define ICIKT_CNT_XTIE 4     /* count_rank_tie(x): ntie, t0, t1 (:102-118) */
#define ICIKT_CNT_YTIE 5
#define ICIKT_CNT_X0 6
#define ICIKT_CNT_X1 7
#define ICIKT_CNT_Y0 8
#define ICIKT_CNT_Y1 9
#define ICIKT_CNT_TOT 10     /* n(n-1)/2 (:280) */
#define ICIKT_CNT_FIELDS 11

/* kernel ids for icikt_kernel_ms */
#define ICIKT_K_PREPARE 0  /* per-column rank pre-pass */
#define ICIKT_K_PAIRS 1    /* pair kernel (discordance / joint-tie counting) */
#define ICIKT_K_EPILOGUE 2 /* tau / p-value epilogue */
#define ICIKT_K_COUNT 3

typedef struct icikt_ctx icikt_ctx;

/* The caller's matrix as the *_in host entries read it: n_feat x n_samp cells of `dtype` at `data`, ld in ELEMENTS.
 * The cells are converted as C converts them, (double)v: float32 and int32 exactly, int64 to the nearest double (ties
 * to even above 2^53, as numpy's astype), a float64 cell bit for bit (NaN payloads kept: NA_real_ stays NA_real_), a
 * float32 NaN to some float64 NaN.  global_na is applied after the conversion, in float64. */
#define ICIKT_DTYPE_F64 0
#define ICIKT_DTYPE_F32 1
#define ICIKT_DTYPE_I32 2
#define ICIKT_DTYPE_I64 3
#define ICIKT_ORDER_COL 0   /* element (r, c) at data[r + c*ld], ld >= n_feat (the _f64 entries' layout) */
#define ICIKT_ORDER_ROW 1   /* element (r, c) at data[r*ld + c], ld >= n_samp                            */
typedef struct { const void *data; int dtype; int order; int64_t ld; } icikt_input;

/* The caller's matrix as the *_csc host entries read it: compressed-sparse-column, columns = samples as everywhere
 * (scipy.sparse.csc_matrix's data / indices / indptr; R's dgCMatrix x / i / p; the transpose of a cells x genes CSR
 * matrix).  An entry given a view V returns what its _f64 twin returns on the dense column-major float64 matrix M with
 *   M[r, c] = (double)values[k]   if column c has an entry k (indptr[c] <= k < indptr[c + 1]) with indices[k] == r,
 *   M[r, c] = fill                otherwise.
 * The conversion is icikt_input's, (double)v; a float64 cell and `fill` travel as 64 bits (NA_real_ stays NA_real_, -0.0
 * stays -0.0).  Explicitly stored zeros and NaNs are ordinary entries; the indices of a column may come in any order.
 * global_na is applied afterwards, in float64, by the pre-pass, as for a dense matrix -- with the default global_na
 * (NA, Inf, 0) and fill = 0 a CSC matrix is "the non-missing values, column by column".  M exists on the device only:
 * what crosses PCIe is values, indices and indptr, and a kernel (icikt_scatter_csc_dev's) writes M there.
 * Malformed input is an argument error (ICIKT_E_INVALID, the message names the argument, the context stays usable),
 * never a device fault.  Checked on the host before the first copy: a null view, null arrays with entries, an unknown
 * dtype or index_type, indptr[0] < 0, indptr decreasing.  Checked on the device, since the host never scans the
 * entries: a row index outside [0, n_feat), and two entries of one column with the same row ("duplicate entry
 * (sum_duplicates)": scipy would sum them, the library refuses).  The kernel stores nothing through an entry it
 * rejects and records one of them (which one is unspecified); the call fails once its stream has drained, and the
 * caller's result arrays may then hold partial results, as after any failed call. */
#define ICIKT_INDEX_I32 0
#define ICIKT_INDEX_I64 1
typedef struct {
  const void *values;   /* nnz cells of `dtype` (ICIKT_DTYPE_F64 / F32 / I32 / I64) */
  const void *indices;  /* nnz row (feature) indices of `index_type`, each in [0, n_feat) */
  const void *indptr;   /* n_samp + 1 offsets of `index_type`: column c's entries are [indptr[c], indptr[c+1]) */
  int dtype, index_type;
  double fill;          /* every cell without an entry holds this value, bit for bit (0.0 = scipy's toarray) */
} icikt_csc_input;

int icikt_version(void);
/* Number of visible HIP devices (0 and ICIKT_E_NO_DEVICE when none). */
int icikt_device_count(int *count);

int icikt_ctx_create(int device, icikt_ctx **ctx);
void icikt_ctx_destroy(icikt_ctx *ctx);
const char *icikt_last_error(const icikt_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own;
 * NULL selects HIP's default (null) stream.  icikt_ctx_use_own_stream() switches back. */
int icikt_ctx_set_stream(icikt_ctx *ctx, void *hip_stream);
int icikt_ctx_use_own_stream(icikt_ctx *ctx);
int icikt_sync(icikt_ctx *ctx);

/* ---- device-resident path (what bench.py and the multi-GPU driver call) -------------------- */

/* Stream contract.  The context's stream is its own (non-blocking) one, or the caller's after icikt_ctx_set_stream.
 * A device-resident call is work on that stream at the place of the call: it reads its device arguments and the
 * context's state no earlier, has written its device results no later, and never touches them from another stream.
 * Work the caller enqueues on the same stream before or behind the call needs no other ordering (tests/
 * test_gpu_caller_stream.py holds every call below to that).  Which calls return before the stream has reached them:
 *   return at once     icikt_prepare_dev, icikt_prepare_cols_dev, icikt_expand_cols_dev, icikt_convert_dev,
 *                      icikt_set_pairs_combn, and icikt_run_dev for a pair list it has run before -- whatever the
 *                      flags, with the one exception below
 *   synchronise        icikt_run_dev, the first run behind each pre-pass, for columns of 14 273 to 65 535 rows: the
 *                      column statistics that size the pair kernel are read back once per prepared matrix (not with
 *                      ICIKT_FLAG_REUSE_COUNTS on valid counts, not for shorter or wide columns);
 *                      icikt_run_dev, the first run after icikt_set_pairs / icikt_set_pairs_combn (columns up to
 *                      65 535 rows): the task list is built on the host and uploaded;
 *                      icikt_set_pairs (the upload of the list); icikt_scatter_csc_dev (it reports malformed input);
 *                      icikt_kernel_ms, icikt_reset_timers, and a timed call that finds 256 timed launches of its
 *                      kernel unread; icikt_sync
 *   may synchronise    any call that has to grow a workspace: the first of its shape on the context (hipMalloc).
 * icikt_ctx_set_stream and icikt_ctx_use_own_stream wait for the stream the context leaves, so what was enqueued there
 * is complete before the first call on the new stream; icikt_ctx_destroy waits for the stream the context is on before
 * it frees anything, and never destroys a caller's stream.  The host entries (icikt_*_f64 / _in / _csc) take host
 * arrays: their transfers and kernels start behind what the context's stream already holds, and they return when their
 * results are in the caller's arrays. */

/* Per-column pre-pass over a DEVICE matrix: NA bitsets, fill value min-0.1 (src/kendallc.cpp:214-219),
 * stable argsort + dense tie groups (sortedIndex/compare_self, :5-31), tie sums (count_rank_tie).
 * Asynchronous on the context's stream.  dX must stay valid until the stream reaches this point. */
int icikt_prepare_dev(icikt_ctx *ctx, const double *dX, int64_t n_feat, int64_t n_samp, int64_t ld,
                      uint32_t flags);

/* Column-sharded pre-pass for multi-rank use: the prepared state is allocated for alloc_cols >= n_samp
 * columns (so that every rank's slice has the same size) but only columns [col_begin, col_end) are computed.
  * The caller then all-gathers the column slices of the two arrays of icikt_prep_arrays() that carry the information
 * (see below) across ranks (RCCL all-gather) and rebuilds the rest for the received columns before icikt_run_dev().
 * Array i is alloc_cols * bytes_per_col[i] bytes; a rank's columns are one contiguous slice of it provided col_begin is
 * even and col_end is even or n_samp (some arrays interleave column pairs; other ranges are refused), so give
 * every rank an even number of columns. */
#define ICIKT_PREP_ARRAYS 5
int icikt_prepare_cols_dev(icikt_ctx *ctx, const double *dX, int64_t n_feat, int64_t n_samp, int64_t ld,
                           int64_t col_begin, int64_t col_end, int64_t alloc_cols, uint32_t flags);
/* The same from a HOST matrix: columns [col_begin, col_end) are copied to the device in chunks that overlap
 * their pre-pass (a rank uploads 1 / world of the matrix).  Returns when X has been read. */
int icikt_prepare_cols_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                           int64_t col_begin, int64_t col_end, int64_t alloc_cols, uint32_t flags);
int icikt_prep_arrays(icikt_ctx *ctx, void **ptrs, int64_t *bytes_per_col);
/* ICIKT_PREP_ORDER (the descending permutation) and ICIKT_PREP_META (per column: missing-row, fill-group and
 * group-start bitsets + the column's statistics) carry the information: 24 KB per column of 10 000 rows, two
 * collectives.  Everything else -- ICIKT_PREP_REC, ICIKT_PREP_HIROW, ICIKT_PREP_TGROUPS (exposed for inspection: 80 KB
 * per column; a rec / hirow block has n_pad + 8 rows, row n_pad the guard row of the step records) and the state that is
 * not exposed (per-row tie-group indices, the tie program and its step records, the 32-bit copy of the order that long columns keep) -- is a function of a column's order
 * and group starts: icikt_expand_cols_dev() rebuilds it for the received columns [col_begin, col_end). */
#define ICIKT_PREP_ORDER 0
#define ICIKT_PREP_REC 1
#define ICIKT_PREP_HIROW 2
#define ICIKT_PREP_META 3
#define ICIKT_PREP_TGROUPS 4
int icikt_expand_cols_dev(icikt_ctx *ctx, int64_t col_begin, int64_t col_end, uint32_t flags);

/* Pair list (HOST arrays, copied).  Mirrors setup_comparisons' output order (R/kendalltau.R:181-278). */
int icikt_set_pairs(icikt_ctx *ctx, const int32_t *pi, const int32_t *pj, int64_t n_pairs);
/* Pairs [begin, end) of utils::combn(n_samp, 2) order: (0,1),(0,2)...(0,S-1),(1,2)... (R/kendalltau.R:189).
 * This is how ranks shard the upper triangle (reference: ceiling(n_todo/ncore) chunks, :250-255). */
int icikt_set_pairs_combn(icikt_ctx *ctx, int64_t n_samp, int64_t begin, int64_t end);
/* Number of pairs currently set. */
int64_t icikt_num_pairs(const icikt_ctx *ctx);

/* Pair kernel + epilogue into DEVICE buffers: d_out4 [P*4] doubles, d_counts [P*ICIKT_CNT_FIELDS]
 * int64 or NULL, d_reasons [P] int32 or NULL.  Asynchronous on the context's stream. */
int icikt_run_dev(icikt_ctx *ctx, int perspective, int alternative, int continuity, uint32_t flags,
                  double *d_out4, int64_t *d_counts, int32_t *d_reasons);

/* Accumulated HIP-event time (ms) and launch count of one kernel since the last reset; needs
 * ICIKT_FLAG_TIMING on the calls being measured.  Synchronises the stream. */
int icikt_kernel_ms(icikt_ctx *ctx, int kernel, double *ms, int64_t *launches);
int icikt_reset_timers(icikt_ctx *ctx);

/* ---- host-buffer path (what the R .Call glue binds) ----------------------------------------- */

/* ici_split() replacement (R/kendalltau.R:280-308): H2D, pre-pass, pair kernel, epilogue, D2H.
 * pi == NULL means all C(n_samp, 2) pairs in combn order.  counts / reasons may be NULL. */
int icikt_pairs_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                    const int32_t *pi, const int32_t *pj, int64_t n_pairs, int perspective,
                    int alternative, int continuity, uint32_t flags, double *out4, int64_t *counts,
                    int32_t *reasons);

/* ici_kt() replacement for one pair of host vectors of equal length n (the caller checks lengths,
 * src/kendallc.cpp:168-170). */
int icikt_pair_f64(icikt_ctx *ctx, const double *x, const double *y, int64_t n, int perspective,
                   int alternative, int continuity, uint32_t flags, double *out4, int64_t *counts,
                   int32_t *reason);

/* ---- the whole matrix behind one call (what the R glue binds for ici_kendalltau(return_matrix = TRUE)) ----------
 *
 * ici_kendalltau() below its argument checks (R/kendalltau.R:117-176), with NOTHING left to the host:
 *   setup_missing_matrix (R/utils.R:1-23)     global_na is applied by the pre-pass while it reads X: a cell is
 *                                             excluded if it is NaN and global_na holds a NaN, infinite and global_na
 *                                             holds an Inf, or == any other global_na value (at most 32 distinct ones:
 *                                             ICIKT_E_INVALID beyond; the front-ends mask such a matrix themselves).  The
 *                                             masked copy `exclude_data` (R/kendalltau.R:119-121) never exists.  A
 *                                             NaN in X is missing for ici_kt whatever global_na says (Rcpp is_na,
 *                                             src/kendallc.cpp:181) but counts as excluded only under the rule, as in R.
 *   ici_split over the pair list (:158)       pi == NULL: all C(n_samp, 2) pairs in combn order; else the caller's list
 *                                             (setup_comparisons' include_only filter, self pairs when !diag_good)
 *   scale_and_reshape (:357-421)              cor = raw / max(taumax, na.rm = TRUE) over the computed pairs when
 *                                             scale_max; diag_good: raw = cor = n_good / max(n_good), pvalue 0,
 *                                             taumax 1, completeness = n_good / n_feat on the diagonal, n_good =
 *                                             colSums(!exclude_loc); symmetric fill, cells never computed stay 0
 * out5: [5][n_samp][n_samp] doubles -- cor, raw, pvalue, taumax, completeness (symmetric: either major order).
 * keep (optional): [n_samp][n_feat] bytes, 1 = not excluded -- the reference's `keep = t(!exclude_loc)` (:417).
 * reason_counts (optional): [5] pairs per reason code ICIKT_OK .. ICIKT_NA_TIES_EQ_TOTAL; the host raises the
 * reference's warning once per pair of codes 2..4, as ici_split does.  Same error contract as icikt_pairs_f64. */
int icikt_matrix_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                     const double *global_na, int n_global_na, const int32_t *pi, const int32_t *pj, int64_t n_pairs,
                     int perspective, int alternative, int continuity, uint32_t flags, int scale_max, int diag_good,
                     double *out5, uint8_t *keep, int64_t *reason_counts);

/* ---- top-k partners per sample, chosen on the device -----------------------------------------------------------
 *
 * For every column (sample) c of X its k partners j != c with the largest ICI-Kendall-tau, each with the five values
 * icikt_matrix_f64 reports for that pair -- without anything of size n_samp^2 on the device or the host: the combn
 * triangle runs through the pair engine in blocks of whole rows, and a selection kernel folds each block into the
 * columns' lists (device memory: the prepared matrix, one block's buffers and 88 n_samp k bytes of lists).
 *   candidates   all C(n_samp, 2) pairs, each seen from both of its columns; never the diagonal; a pair whose raw is
 *                NA (reason codes 1..4) is no candidate for either column
 *   order        raw descending in the total order of the doubles' bits (so -0.0 sorts below +0.0), ties by the smaller
 *                partner index: a pure function of the set of (raw, partner), whatever the blocks
 *   values       cor, raw, pvalue, taumax, completeness; cor = scale_max ? raw / max(taumax, na.rm = TRUE) : raw over
 *                ALL computed pairs (-Inf when there is none), bit for bit the cell of icikt_matrix_f64's matrices;
 *                the ranking is by raw whatever scale_max says
 *   padding      a column with fewer than k valid partners: idx -1 and R's NA_real_ in all five values
 * idx: [n_samp][k]; out5k: [5][n_samp][k]; n_valid (optional): [n_samp] real partners per column; max_taumax
 * (optional): the scale's denominator; reason_counts (optional): [5] pairs per reason code, as icikt_matrix_f64.
 * 1 <= k <= ICIKT_TOPK_MAX (k > n_samp - 1 means padding); n_samp <= ICIKT_TOPK_MAX_SAMPLES, so that pair indices
 * stay 32-bit (ICIKT_E_INVALID beyond, the message names the limit); n_feat as icikt_run_dev takes it; global_na as
 * icikt_matrix_f64.  Like icikt_pairs_complete_f64 the call leaves neither a prepared matrix nor a pair list behind:
 * icikt_run_dev answers ICIKT_E_STATE and icikt_num_pairs -1 afterwards.  A call refused at its argument checks
 * touches nothing.  With ICIKT_FLAG_TIMING the selection kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_topk_in / icikt_topk_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_TOPK_MAX 256
#define ICIKT_TOPK_MAX_SAMPLES 65535
int icikt_topk_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld, const double *global_na,
                   int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags,
                   int scale_max, int32_t *idx, double *out5k, int32_t *n_valid, double *max_taumax,
                   int64_t *reason_counts);

/* ---- every pair past a threshold, compacted on the device ------------------------------------------------------
 *
 * The edge list of a correlation network: every pair i < j of columns of X whose values pass `rule`, with the five
 * values icikt_matrix_f64 reports for that pair -- without anything of size n_samp^2 on the device or the host.  The
 * combn triangle runs through the pair engine in blocks of whole rows, as for icikt_topk_f64, and an ordered stream
 * compaction appends each block's matching records to the kept ones (device memory: the prepared matrix, one block's
 * buffers and 48 min(max_edges, C(n_samp, 2)) bytes of kept edges).
 *   rule         a pair is an edge iff its raw is not NA (reason code 0) and every bound of the rule that is not NaN
 *                holds, as a plain IEEE comparison of doubles: raw >= min_raw (fabs(raw) >= min_raw when absolute != 0),
 *                pvalue <= max_pvalue, completeness >= min_completeness.  A NaN pvalue therefore fails a p-value bound
 *                and passes when there is none.  The diagonal is never an edge.  The bounds apply to RAW, never to cor:
 *                cor's denominator, max(taumax) over all pairs, is known only after the last block.
 *   order        combn order: i ascending, then j ascending.  The order is strict, so the output is a pure function of
 *                the input, whatever the block cut.
 *   values       ei / ej: the pair's columns; out5e: [5][max_edges] planes cor, raw, pvalue, taumax, completeness;
 *                cor = scale_max ? raw / max(taumax, na.rm = TRUE) : raw over ALL computed pairs, bit for bit the cell
 *                of icikt_matrix_f64's matrices
 *   capacity     *n_edges: the number of matching pairs, ALL of them; the first min(*n_edges, max_edges) are written,
 *                the slots behind them are left untouched.  *n_edges > max_edges is no error: call again with room.
 *                max_edges = 0 (ei, ej, out5e may then be null) only counts.
 * degree (optional): [n_samp] matching pairs that contain the column, all of them whatever max_edges; max_taumax and
 * reason_counts (optional): as icikt_topk_f64.  n_samp <= ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID beyond, the message
 * names the limit); n_feat, global_na, the state the call leaves behind (none: icikt_run_dev answers ICIKT_E_STATE and
 * icikt_num_pairs -1) and the refusal of bad arguments before anything -- the context or an output -- is touched: as
 * icikt_topk_f64.  With ICIKT_FLAG_TIMING the compaction kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_edges_in / icikt_edges_csc: the same on a typed view / a CSC view of the matrix (below). */
typedef struct icikt_edge_rule {
  double min_raw;           /* NaN: no bound.  raw >= min_raw; with absolute != 0: fabs(raw) >= min_raw */
  double max_pvalue;        /* NaN: no bound.  pvalue <= max_pvalue */
  double min_completeness;  /* NaN: no bound.  completeness >= min_completeness */
  int absolute;
} icikt_edge_rule;
int icikt_edges_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld, const double *global_na,
                    int n_global_na, const icikt_edge_rule *rule, int perspective, int alternative, int continuity,
                    uint32_t flags, int scale_max, int64_t max_edges, int32_t *ei, int32_t *ej, double *out5e,
                    int64_t *n_edges, int64_t *degree, double *max_taumax, int64_t *reason_counts);

/* ---- per-sample median ICI-Kendall-tau within classes, reduced on the device --------------------------------------
 *
 * The quality-control figure the matrix is made for: for every column (sample) s of X the median of raw (and of cor)
 * over the other samples of its class -- without anything of size n_samp^2 on the device or the host, and without
 * computing a pair that crosses classes.  The within-class pairs run through the pair engine in blocks; a kernel
 * keeps each pair's raw as a sortable 64-bit key, and after the last block a selection kernel finds every sample's
 * median by a radix select over its partners' keys.
 *   classes      cls[s] in 0 .. n_class - 1 per sample; cls == NULL: one class (n_class is then ignored).  A class may
 *                be empty.  A class index outside the range is ICIKT_E_INVALID, found before anything is touched.
 *   pairs        only pairs i < j with cls[i] == cls[j], listed class by class in class-index order, inside a class in
 *                combn order over its members by ascending sample index (one class: the combn triangle)
 *   partners     of sample s: the other members of its class whose pair with s has reason code 0 (raw is not NA);
 *                n_valid[s] is their count
 *   med_raw      R's median(raw, na.rm = TRUE) over the partners: the middle value, or the mean of the two middle
 *                values, a zero returned as +0; NA_real_ (bits 0x7FF00000000007A2) when n_valid[s] == 0, which covers
 *                singleton classes
 *   med_cor      the same rule on a / m (and b / m) for the one or two middle raw values a (and b), m = scale_max ?
 *                max(taumax, na.rm = TRUE) over the COMPUTED pairs : 1 -- the operands are bit for bit the cor cells of
 *                icikt_matrix_f64 called with that pair list.  m is the WITHIN-CLASS maximum, not the maximum over all
 *                C(n_samp, 2) pairs; med_raw does not depend on it.  Without scale_max med_cor equals med_raw.
 * med2: [2][n_samp], cor then raw; n_valid (optional): [n_samp]; max_taumax (optional): m, -Inf when no pair was computed;
 * reason_counts (optional): [5] computed pairs per reason code.  n_samp <= ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID
 * beyond, the message names the limit); n_feat, global_na, the state the call leaves behind (none: icikt_run_dev
 * answers ICIKT_E_STATE and icikt_num_pairs -1) and the refusal of bad arguments before anything -- the context or an
 * output -- is touched: as icikt_topk_f64.
 * One class runs in blocks of whole combn rows (the tkblock budget, as icikt_topk_f64); several classes as an explicit
 * pair list in slices of the same budget, each slice's pi / pj generated on the host when its turn comes (host memory
 * O(block)).  Device memory: the prepared matrix, one block's buffers, 8 bytes per computed pair for the kept keys
 * (sum over the classes of m (m - 1) / 2 pairs; one class of 65 535 samples: 17 GB) and 36 n_samp bytes of index
 * arrays (position in class, class size, first pair of the class as int64: 16) and results (20); a failed allocation
 * is ICIKT_E_HIP.
 * With ICIKT_FLAG_TIMING the keep and select kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_class_medians_in / icikt_class_medians_csc: the same on a typed view / a CSC view of the matrix (below). */
int icikt_class_medians_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                            const double *global_na, int n_global_na, const int32_t *cls, int n_class, int perspective,
                            int alternative, int continuity, uint32_t flags, int scale_max, double *med2,
                            int32_t *n_valid, double *max_taumax, int64_t *reason_counts);

/* ---- exact quantiles and a histogram of raw over all pairs, reduced on the device ---------------------------------
 *
 * The distribution of the pair values: from a features x samples matrix the exact quantiles (R's quantile(type = 7))
 * and a histogram of raw over all C(n_samp, 2) pairs -- the cut-off icikt_edges_f64 is called with, the picture a
 * quality-control report draws -- without anything of size n_samp^2 on the host or as five planes on the device.  The
 * whole combn triangle runs through the pair engine in blocks of whole rows (the tkblock budget, as icikt_topk_f64).
 *   groups       n_group = 1 when cls == NULL (n_class is then ignored), else 3: group 0 every pair, group 1 the pairs
 *                with cls[i] == cls[j], group 2 the pairs with cls[i] != cls[j].  cls[s] in 0 .. n_class - 1, checked
 *                as icikt_class_medians_f64 checks it.
 *   values       a pair with a non-zero reason code has an NA raw: it is no value and counts in n_na[g]; n_valid[g]
 *                counts the others.  Values are ordered by the sortable key of icikt_class_medians_f64: -0 and +0 are
 *                one value, and a zero comes back as +0.
 *   probs        n_probs (0 .. ICIKT_QUANTILE_MAX_PROBS) doubles in [0, 1], in any order, repeats allowed; NaN or a
 *                value outside is ICIKT_E_INVALID, the message names the index.  n_probs = 0: no quantiles, and nothing
 *                is kept per pair.
 *   breaks       n_breaks = 0 (no histogram), or 2 .. ICIKT_HIST_MAX_BINS + 1 finite, strictly increasing doubles
 *                (else ICIKT_E_INVALID, the message names the index).  The device only compares raw with these values.
 *   order2       [n_group][n_probs][2]: with the v = n_valid[g] values ascending x[1..v], index = 1 + (v - 1) p in
 *                double arithmetic, the order statistics x[floor(index)] and x[ceil(index)]; NA_real_ (bits
 *                0x7FF00000000007A2) twice when v = 0
 *   q2           [2][n_group][n_probs], cor then raw.  raw: a = x[lo], b = x[hi], h = index - lo: a when index == lo or
 *                a == b, else (1 - h) a + h b, every operation rounded on its own (no fused multiply-add), a zero as
 *                +0.  cor: the same rule on a / m and b / m, m = scale_max ? max(taumax, na.rm = TRUE) over all
 *                computed pairs : 1 -- the operands icikt_matrix_f64's cor cells are made of.  NA_real_ when v = 0.
 *   hist         [n_group][n_breaks - 1], numpy.histogram(valid raw, bins = breaks): bin k counts breaks[k] <= raw <
 *                breaks[k + 1], the last bin also raw == breaks[n_breaks - 1]
 *   outside      [n_group][2]: valid raw < breaks[0], valid raw > breaks[n_breaks - 1] (0 without breaks)
 * q2 and order2 are required when n_probs > 0, hist when n_breaks > 0; n_valid, n_na ([n_group] each), outside,
 * max_taumax and reason_counts (as icikt_topk_f64) are optional.  n_samp <= ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID
 * beyond, the message names the limit); n_feat, global_na, the state the call leaves behind (none: icikt_run_dev
 * answers ICIKT_E_STATE and icikt_num_pairs -1) and the refusal of bad arguments before anything -- the context or an
 * output -- is touched: as icikt_topk_f64.  The result is a pure function of the input: integer counts alone, whatever
 * the block cut.
 * Device memory: the prepared matrix, one block's buffers, and with n_probs > 0 8 bytes per pair of the triangle for
 * the kept keys (n_samp = 65 535: 17 GB; group membership is recomputed from a pair's index, not kept); besides that
 * 4 n_samp bytes of class index, 8 n_breaks + 16 (n_breaks + 3) bytes of breaks and totals and 69 KB for the select's
 * targets and digit histograms.  A failed allocation is ICIKT_E_HIP.
 * With ICIKT_FLAG_TIMING the fold and select kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_quantiles_in / icikt_quantiles_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_QUANTILE_MAX_PROBS 32
#define ICIKT_HIST_MAX_BINS 1024
int icikt_quantiles_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                        const double *global_na, int n_global_na, const int32_t *cls, int n_class, int perspective,
                        int alternative, int continuity, uint32_t flags, int scale_max, const double *probs, int n_probs,
                        const double *breaks, int n_breaks, double *q2, double *order2, int64_t *n_valid, int64_t *n_na,
                        int64_t *hist, int64_t *outside, double *max_taumax, int64_t *reason_counts);

/* ---- per-sample median ICI-Kendall-tau to every class, reduced on the device --------------------------------------
 *
 * The other half of icikt_class_medians_f64: for every column (sample) s of X and every class c the median of raw (and
 * of cor) over the members of c -- the table in which a mislabelled or swapped sample correlates better with another
 * class than with its own, and from which an unlabelled sample is assigned to its nearest class -- without anything of
 * size n_samp^2 on the host or as five planes on the device.  The whole combn triangle runs through the pair engine in
 * blocks of whole rows (the tkblock budget, as icikt_topk_f64); a kernel keeps each pair's raw as a sortable 64-bit
 * key, and after the last block a selection kernel finds every cell's median by a radix select over the keys of the
 * sample's pairs with the class's members.
 *   classes      cls[s] in 0 .. n_class - 1 per sample; cls == NULL: one class (n_class is then ignored and the table
 *                has one column).  A class may be empty.  n_class <= 65 535, the second dimension of the select
 *                kernel's grid; beyond it, and for a class index outside the range, ICIKT_E_INVALID before anything is
 *                touched.
 *   partners     of cell (s, c): the members t != s of class c whose pair with s has reason code 0 (raw is not NA);
 *                n_valid[s, c] is their count
 *   med_raw      R's median(raw, na.rm = TRUE) over the partners, by icikt_class_medians_f64's rule: the middle value, or
 *                the mean of the two middle values, a zero returned as +0; NA_real_ (bits 0x7FF00000000007A2) when
 *                n_valid[s, c] == 0: an empty class, the sample's own singleton class, NA pairs alone
 *   med_cor      the same rule on a / m (and b / m) for the one or two middle raw values a (and b), m = scale_max ?
 *                max(taumax, na.rm = TRUE) over ALL C(n_samp, 2) pairs : 1 -- the operands are bit for bit the cor cells
 *                of icikt_matrix_f64 over all pairs.  Without scale_max med_cor equals med_raw.
 * The own-class column c = cls[s] carries the med_raw and n_valid of icikt_class_medians_f64 bit for bit; with one class
 * med_cor agrees as well, both entries then scaling by the same m.
 * med2: [2][n_class][n_samp], cor then raw, the sample index fastest (column-major n_samp x n_class planes); n_valid
 * (optional): [n_class][n_samp] in the same layout; max_taumax (optional): m, -Inf when no pair had one; reason_counts
 * (optional): [5] pairs of the triangle per reason code.  n_samp <= ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID beyond, the
 * message names the limit); n_feat, global_na, the state the call leaves behind (none: icikt_run_dev answers
 * ICIKT_E_STATE and icikt_num_pairs -1) and the refusal of bad arguments before anything -- the context or an output --
 * is touched: as icikt_topk_f64.
 * Device memory: the prepared matrix, one block's buffers, 8 bytes per pair of the triangle for the kept keys (n_samp =
 * 65 535: 17 GB), 4 (n_samp + n_class + 1) bytes of member list and class ranges and 20 n_samp n_class bytes of
 * results; a failed allocation is ICIKT_E_HIP.
 * With ICIKT_FLAG_TIMING the keep and select kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_class_matrix_in / icikt_class_matrix_csc: the same on a typed view / a CSC view of the matrix (below). */
int icikt_class_matrix_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                           const double *global_na, int n_global_na, const int32_t *cls, int n_class, int perspective,
                           int alternative, int continuity, uint32_t flags, int scale_max, double *med2,
                           int32_t *n_valid, double *max_taumax, int64_t *reason_counts);

/* ---- multiple-testing adjustment of the p-values of all pairs, on the device ----------------------------------------
 *
 * The step that follows every all-pairs call: R's p.adjust(p, method) over the p-values of all C(n_samp, 2) pairs, and
 * from it the number of pairs rejected at each alpha and the raw p-value to cut at -- without anything of size n_samp^2
 * on the host or as five planes on the device.  The whole combn triangle runs through the pair engine in blocks of
 * whole rows (the tkblock budget, as icikt_topk_f64); a kernel keeps each pair's p-value as a sortable 64-bit key, and
 * after the last block the device sorts the keys (a radix sort across the chip), scans them and compacts the table.
 *   tests        the pairs i < j whose reason code is 0 and whose p-value is not NaN; m = n_tests[0] is their count,
 *                n_tests[1] the count of the other pairs.  (Two-row input gives reason-free pairs with a NaN p: no
 *                tests, as p.adjust drops an NA.)
 *   method       ICIKT_ADJUST_BONFERRONI, _HOLM, _HOCHBERG or _BH.  With the m p-values ascending p(1) <= .. <= p(m), i
 *                the 1-based position, the adjusted values in that order are R's p.adjust, one IEEE double operation at
 *                a time:
 *                  bonferroni  min(1, m p(i))
 *                  holm        min(1, max over j <= i of (m + 1 - j) p(j))
 *                  hochberg    min(1, min over j >= i of (m + 1 - j) p(j))
 *                  BH          min(1, min over j >= i of (m / j) p(j)), the quotient rounded first, then the product
 *                m, j and m + 1 - j are exact as doubles (m < 2^31); there is one division and one multiplication and no
 *                addition of doubles, so nothing contracts into a fused multiply-add; maxima and minima are exact.  The
 *                result is defined to the bit.  For all four methods the sequence is non-decreasing and constant on a
 *                run of equal p-values: the adjusted value is a function of the value of p alone.
 *   alpha        n_alpha (1 .. ICIKT_ADJUST_MAX_ALPHA) doubles in [0, 1]; NaN or a value outside is ICIKT_E_INVALID, the
 *                message names the index
 *   n_rejected   [n_alpha] the tests whose adjusted value is <= alpha[a]
 *   p_cutoff     [n_alpha] p(n) with n = n_rejected[a], NA_real_ (bits 0x7FF00000000007A2) when n = 0.  Every method
 *                rejects a lower set of the order, so adjusted <= alpha[a] iff pvalue <= p_cutoff[a] for every test:
 *                icikt_edges_f64 with rule.max_pvalue = p_cutoff[a] selects exactly the rejected pairs.
 *   table        [2][max_table]: the distinct p-values among the first max over a of n_rejected[a] sorted positions,
 *                ascending, in plane 0 (a zero as +0), their adjusted values in plane 1.  *n_table: the number of
 *                distinct values, ALL of them; the first min(*n_table, max_table) are written, the slots behind them are
 *                left untouched.  *n_table > max_table is no error: call again with room.  max_table = 0 (table may then
 *                be null) only counts.
 * Without a test (m = 0; n_samp of 0 or 1 included) every n_rejected is 0, every p_cutoff NA_real_ and *n_table 0.
 * n_tests, n_rejected, p_cutoff and n_table are required, table with max_table > 0; max_taumax and reason_counts (as
 * icikt_topk_f64, over all pairs) are optional.  A bad method, n_alpha, alpha, a negative max_table, a null output:
 * ICIKT_E_INVALID.  n_samp <= ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID beyond, the message names the limit); n_feat,
 * global_na, the state the call leaves behind (none: icikt_run_dev answers ICIKT_E_STATE and icikt_num_pairs -1) and the
 * refusal of bad arguments before anything -- the context or an output -- is touched: as icikt_topk_f64.  The result is
 * a pure function of the input: a sorted multiset of keys and scans of exact operations, whatever the block cut, the
 * sort's tile or the grid.
 * Device memory: the prepared matrix, one block's buffers, 16 bytes per pair of the triangle for the kept keys and the
 * sort's second plane (n_samp = 65 535: 34 GB), 2 KB per tile of the sort (at most 65 536 tiles), 8 bytes per 1 024
 * pairs for the scans and 16 min(max_table, pairs) bytes of table.  A failed allocation is ICIKT_E_HIP.
 * With ICIKT_FLAG_TIMING the fold, sort, scan and table kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_padjust_in / icikt_padjust_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_ADJUST_BONFERRONI 0
#define ICIKT_ADJUST_HOLM 1
#define ICIKT_ADJUST_HOCHBERG 2
#define ICIKT_ADJUST_BH 3
#define ICIKT_ADJUST_MAX_ALPHA 16
int icikt_padjust_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                      const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                      uint32_t flags, int method, const double *alpha, int n_alpha, int64_t max_table, int64_t *n_tests,
                      int64_t *n_rejected, double *p_cutoff, double *table, int64_t *n_table, double *max_taumax,
                      int64_t *reason_counts);

/* ---- maximum spanning forest of the samples: single-linkage clustering, on the device -------------------------------
 *
 * Clustering the samples by their correlation, and the question of a correlation network "at which cut-off does it
 * fall apart, and into which clusters": single-linkage clustering is the maximum spanning tree of the complete graph
 * weighted by raw, and one tree gives the dendrogram and the connected components of the thresholded network at EVERY
 * cut-off -- without anything of size n_samp^2 on the host or as five planes on the device.  The whole combn triangle
 * runs through the pair engine in blocks of whole rows (the tkblock budget, as icikt_topk_f64); a kernel keeps each
 * pair's raw as a sortable 64-bit key, and after the last block Boruvka rounds run over the kept keys: a kernel finds
 * every sample's best edge out of its component, the host (O(n_samp) per round) picks each component's best, merges
 * and uploads the new components.  Only comparisons enter, no addition of doubles: the result is defined to the bit.
 * (Complete and average linkage need n_samp - 1 dependent updates of an n_samp x n_samp table: icikt_hclust_f64, below.)
 *   candidate    a pair i < j is a candidate edge iff its raw is not NA (reason code 0) and, when min_raw is not NaN,
 *                raw >= min_raw -- a plain IEEE comparison, as icikt_edge_rule's
 *   order        the STRICT EDGE ORDER: the larger raw first, -0 equal to +0; equal raw by the smaller combn index (i
 *                ascending, then j ascending).  The order is total, so the maximum spanning forest under it is unique:
 *                a pure function of the input, whatever the block cut, the round structure or the launch geometry.
 *   ti, tj       [n_samp - 1] the forest's edges i < j IN THE STRICT ORDER: Kruskal's order, which is the single-linkage
 *                merge order.  *n_tree of them are written, the slots behind them are left untouched.
 *   out5t        [5][n_samp - 1] planes (n_samp - 1 apart): cor, raw, pvalue, taumax, completeness of each edge, bit for
 *                bit the cells of icikt_matrix_f64; cor = scale_max ? raw / max(taumax, na.rm = TRUE) over ALL
 *                C(n_samp, 2) pairs : raw
 *   component    [n_samp] the sample's connected component in the candidate graph, the components numbered 0, 1, .. in
 *                order of their smallest sample.  A sample all of whose pairs are NA or below min_raw -- a constant or
 *                all-missing column -- is a component of its own.  *n_tree + *n_components == n_samp always.
 *   n_rounds     the rounds run (a diagnostic): at most 17, since the components that still have a candidate at least
 *                halve per round.  A round that merges nothing while candidates exist, or counts that do not add up, is
 *                ICIKT_E_STATE with a message -- never a loop.
 * ti, tj and out5t are required for n_samp > 1, component for n_samp > 0, n_tree, n_components and n_rounds always;
 * max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are optional.  n_samp <= ICIKT_TOPK_MAX_SAMPLES
 * (ICIKT_E_INVALID beyond, the message names the limit); n_feat, global_na, the state the call leaves behind (none:
 * icikt_run_dev answers ICIKT_E_STATE and icikt_num_pairs -1) and the refusal of bad arguments before anything -- the
 * context or an output -- is touched: as icikt_topk_f64.
 * Device memory: the prepared matrix, one block's buffers, 8 bytes per pair of the triangle for the kept keys (n_samp =
 * 65 535: 17 GB) and 24 n_samp bytes of component labels, live flags and candidates; a failed allocation is ICIKT_E_HIP.
 * With ICIKT_FLAG_TIMING the keep kernel, the rounds and the pair run over the tree's edges are accounted under
 * ICIKT_K_EPILOGUE.
 * icikt_mst_in / icikt_mst_csc: the same on a typed view / a CSC view of the matrix (below). */
int icikt_mst_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld, const double *global_na,
                  int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  double min_raw, int32_t *ti, int32_t *tj, double *out5t, int64_t *n_tree, int32_t *component,
                  int64_t *n_components, int32_t *n_rounds, double *max_taumax, int64_t *reason_counts);

/* ---- complete, average and single linkage of the samples, on the device ---------------------------------------------
 *
 * The sample dendrogram and heatmap ordering by the methods R's hclust ("complete") and scipy ("average") default to,
 * without anything of size n_samp^2 on the host or as five planes on the device.  The whole combn triangle runs through
 * the pair engine in blocks of whole rows (the tkblock budget, as icikt_topk_f64); a kernel keeps each pair's raw as a
 * sortable 64-bit key; after the last block a kernel expands the keys into a symmetric n_samp x n_samp table, and
 * n_samp - 1 steps of three short launches each (pick the best pair, update the merged row and column, rescan the rows
 * whose cached neighbour went away) are queued without a host wait.  Only the merge records come back.
 *   similarity   of two samples: the pair's raw, -0 equal to +0; a pair with a reason code or an NA raw has none (NA)
 *   clusters     a cluster lives in the slot of its smallest sample; slots a < b merge into a
 *   NA           the merged cluster's similarity to a cluster k is NA if either old one is: two clusters are mergeable
 *                exactly when every sample pair across them has a raw
 *   method       ICIKT_HCLUST_COMPLETE: the smaller of the two old similarities; ICIKT_HCLUST_SINGLE: the larger;
 *                ICIKT_HCLUST_AVERAGE: (n_a w_a + n_b w_b) / (n_a + n_b) in IEEE doubles, each of the two products, the
 *                two sums and the division rounded once, no fused operation
 *   order        each step merges the best live pair in the STRICT ORDER: the larger similarity first, then the smaller
 *                a, then the smaller b.  The order is total: the result is a pure function of the input, whatever the
 *                block cut or the launch geometry.
 *   end          at the first step whose best similarity is NA or, when min_raw is not NaN, below min_raw (a plain IEEE
 *                comparison).  What is left is a forest.
 *   ma, mb       [n_samp - 1] the slots a < b of each merge, in merge order; *n_merges of them are written, the slots
 *                behind them are left untouched (as in msize, mraw, mcor)
 *   msize        [n_samp - 1] the samples of the new cluster
 *   mraw, mcor   [n_samp - 1] the similarity of the merge (-0 as +0) and mcor = scale_max ? mraw / max(taumax, na.rm =
 *                TRUE) over ALL C(n_samp, 2) pairs : mraw
 *   component    [n_samp] the sample's cluster when merging ended, the clusters numbered 0, 1, .. in order of their
 *                smallest sample.  *n_merges + *n_components == n_samp always.
 * ma, mb, msize, mraw and mcor are required for n_samp > 1, component for n_samp > 0, n_merges and n_components always;
 * max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are optional.  Any other method is ICIKT_E_INVALID
 * (the message names `method`); n_samp <= ICIKT_TOPK_MAX_SAMPLES; n_feat, global_na, the state the call leaves behind
 * and the refusal of bad arguments before anything -- the context or an output -- is touched: as icikt_topk_f64.
 * Records that do not add up (n_merges + n_components != n_samp, a >= b, a slot that is no cluster any more, a merge
 * without a similarity or below min_raw, complete or single merges whose similarities increase) are ICIKT_E_STATE with a
 * message -- never a loop.
 * Device memory: the prepared matrix, one block's buffers, 8 bytes per pair of the triangle for the kept keys and 8
 * n_samp^2 bytes for the table (12 n_samp^2 together; n_samp = 65 535: 52 GB) and 40 n_samp bytes of neighbours, flags,
 * sizes, list and records; a failed allocation is ICIKT_E_HIP.  With ICIKT_FLAG_TIMING the keep kernel, the table, the
 * first scan and the steps are accounted under ICIKT_K_EPILOGUE.
 * icikt_hclust_in / icikt_hclust_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_HCLUST_COMPLETE 0
#define ICIKT_HCLUST_AVERAGE 1
#define ICIKT_HCLUST_SINGLE 2
int icikt_hclust_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                     const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                     uint32_t flags, int scale_max, int method, double min_raw, int32_t *ma, int32_t *mb,
                     int32_t *msize, double *mraw, double *mcor, int64_t *n_merges, int32_t *component,
                     int64_t *n_components, double *max_taumax, int64_t *reason_counts);

/* ---- ANOSIM: do the classes separate under ICI-Kt, with a permutation test, on the device --------------------------
 *
 * The question a quality-control run asks once the samples carry class labels: analysis of similarities (Clarke 1993;
 * vegan::anosim) on the dissimilarity 1 - raw, without anything of size n_samp^2 on the host or as five planes on the
 * device.  The whole combn triangle runs through the pair engine in blocks of whole rows (the tkblock budget, as
 * icikt_topk_f64); a kernel keeps each pair's raw as a sortable 64-bit key; after the last block the device sorts a
 * copy of the keys, ranks every pair, and sums the ranks of the within-class pairs of every labelling.
 *   value        a pair i < j is a value iff its raw is not NA (reason code 0); M = n_pairs[0] is their count,
 *                n_pairs[1] the count of the other pairs
 *   order        values compare as their raw does, -0 equal to +0; equal doubles are ties
 *   rank         a value's average rank among the M values in ascending dissimilarity 1 - raw, that is in DESCENDING
 *                raw: R's rank(1 - raw, ties = "average") without the rounding of 1 - raw.  The library works with the
 *                DOUBLED rank r2 = 2 M - lo - hi + 1 (lo: the values below the pair's raw, hi: those at or below it),
 *                an integer in 2 .. 2 M
 *   sums         for a labelling L (a class index per sample) W2(L) is the sum of r2 over the values whose two samples
 *                share a class, nW(L) their count; T2 = M (M + 1) is the sum over all values, nB = M - nW.  Then
 *                  R(L) = (T2 nW - W2 M) / (nW nB M)
 *                exactly: vegan's -diff(tapply(rank, within, mean)) / (length(rank) / 2); without an NA pair M / 2 is
 *                n_samp (n_samp - 1) / 4 as there.  R is UNDEFINED when nW = 0 or nB = 0: one class, singleton classes
 *                only, M = 0, or -- with NA pairs -- a labelling that leaves no within-class value.
 *   cls          [n_samp] the observed labelling, each in 0 .. n_class - 1 (NULL: one class, n_class ignored);
 *                1 <= n_class <= ICIKT_ANOSIM_MAX_CLASSES
 *   perm_cls     [n_perm][n_samp] row-major, the labellings to compare with (the caller's permutations of cls; any
 *                labels in 0 .. n_class - 1 are taken as given), 0 <= n_perm <= ICIKT_ANOSIM_MAX_PERM.  They are read
 *                once, where they lie, and cross to the device in batches of bounded size; every label is checked on
 *                the way: one out of range is ICIKT_E_INVALID, the message names the permutation and the sample.
 *   w2, nw       [1 + n_perm] W2 and nW; index 0 is the observed labelling, index 1 + t permutation t
 *   n_ge         the permutations whose R is defined and >= the observed R, compared EXACTLY by cross-multiplication in
 *                128-bit integers (vegan subtracts sqrt(.Machine$double.eps) because it compares rounded doubles; exact
 *                arithmetic needs no margin).  The p-value is (1 + n_ge) / (1 + n_perm).  0 when the observed R is
 *                undefined.
 *   n_undefined  the permutations without an R; they are not counted as >=
 *   class_w2, class_nw   [n_class] the observed labelling's sums restricted to the values inside class c: class c's
 *                mean within rank is class_w2[c] / (2 class_nw[c])
 * Every sum is below 2^63 (T2 < 2^63 at 65 535 samples).  n_samp of 0 or 1 gives M = 0 and zero sums; it is no error.
 * All outputs but max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are required.  A bad n_class, a label
 * of cls out of range, a negative or too large n_perm, n_perm > 0 with a null perm_cls, a null output: ICIKT_E_INVALID
 * before anything -- the context or an output -- is touched; a label of perm_cls out of range: ICIKT_E_INVALID with
 * the outputs untouched.  n_samp <= ICIKT_TOPK_MAX_SAMPLES; n_feat, global_na and the state the call leaves behind
 * (none): as icikt_topk_f64.  The result is a pure function of the input and the labellings: integer sums, counts and
 * comparisons, whatever the block cut, the sort's tile, the batch, the strip or the grid.
 * Device memory: the prepared matrix, one block's buffers, 24 bytes per pair of the triangle for the kept keys, their
 * sorted copy and the sort's second plane, which takes the ranks (n_samp = 65 535: 51 GB), 2 KB per tile of the sort,
 * and a batch of labels at two bytes each (64 MB unless the anoperms plan key says otherwise).  A failed allocation is
 * ICIKT_E_HIP.  With ICIKT_FLAG_TIMING the keep, count, sort, rank and permutation kernels are accounted under
 * ICIKT_K_EPILOGUE.
 * icikt_anosim_in / icikt_anosim_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_ANOSIM_MAX_PERM 1000000
#define ICIKT_ANOSIM_MAX_CLASSES 65535
int icikt_anosim_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                     const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                     uint32_t flags, const int32_t *cls, int n_class, const int32_t *perm_cls, int64_t n_perm,
                     int64_t *n_pairs, int64_t *w2, int64_t *nw, int64_t *n_ge, int64_t *n_undefined,
                     int64_t *class_w2, int64_t *class_nw, double *max_taumax, int64_t *reason_counts);

/* ---- PERMANOVA: the sums of squared dissimilarities per class, of the observed labelling and of permutations ---------
 *
 * The test of class separation that is reported beside (or instead of) ANOSIM: Anderson 2001, vegan::adonis2,
 * skbio.stats.distance.permanova, on the dissimilarity 1 - raw.  The triangle runs as in icikt_anosim_f64; a pair is a
 * VALUE iff its raw is not NA.  A value's squared dissimilarity is summed as the integer
 *   q = llrint(ldexp(e, 50)),  e = d * d,  d = 1.0 - raw   (IEEE double, one rounding each; round half to even),
 * raw the double of the pair's key (-0 is +0): 0 <= q <= 2^52.  This quantisation is the only inexact step and it is a
 * fixed function of raw (csrc/icikt_fixed.h); everything behind it is an integer sum.  This entry returns integers
 * only; the statistic -- SS_T = Q / (n_samp 2^50), SS_W = sum_c A_c / (n_c 2^50) with n_c the labelling's class sizes,
 * pseudo-F, R2, and the exact comparison of labellings -- is the caller's, in rational arithmetic.
 *   cls, n_class, perm_cls, n_perm   as icikt_anosim_f64; additionally (1 + n_perm) n_class <=
 *                ICIKT_PERMANOVA_MAX_CELLS (the bins come back to the host: 16 bytes per cell in the caller's arrays
 *                and as many in the library's until the call has succeeded)
 *   n_pairs      [2] the values and the NA pairs
 *   q_total      [2] Q, the sum of q over all values, as two limbs: Q = q_total[1] 2^32 + q_total[0]
 *   bins_lo, bins_hi   [(1 + n_perm)][n_class] row-major: A_c of labelling l -- the sum of q over the pairs whose two
 *                samples both have class c under l -- is bins_hi[l n_class + c] 2^32 + bins_lo[l n_class + c].  THE LIMB
 *                RULE: A = hi 2^32 + lo with 0 <= lo < 2^63 and 0 <= hi < 2^52; lo is a sum of low 32-bit halves and
 *                may exceed 2^32.  Row 0 is the observed labelling, row 1 + t permutation t; a class without a sample
 *                has 0
 * WITH AN NA PAIR (n_pairs[1] > 0) no labelling is summed and every bin is 0: the 1 / n_c weights have no meaning on
 * an incomplete class, nothing is imputed and no pair is dropped.  q_total is then the sum over the values, and the
 * labels are still checked.  n_samp of 0 or 1 gives zero sums; it is no error.
 * All outputs but max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are required.  A bad n_class, a label
 * of cls out of range, a negative or too large n_perm, too many cells, n_perm > 0 with a null perm_cls, a null output:
 * ICIKT_E_INVALID before anything -- the context or an output -- is touched; a label of perm_cls out of range:
 * ICIKT_E_INVALID with the outputs untouched.  n_samp <= ICIKT_TOPK_MAX_SAMPLES; n_feat, global_na and the state the
 * call leaves behind (none): as icikt_topk_f64.  The result is a pure function of the input and the labellings, whatever
 * the block cut, the batch, the strip or the grid.
 * Device memory: the prepared matrix, one block's buffers, 16 bytes per pair of the triangle for the kept keys and
 * their q (n_samp = 65 535: 34 GB), and per labelling of a batch 18 n_samp bytes of labels and column sums and
 * 16 n_class bytes of bins (the largest of them at most 64 MB per batch unless the anoperms plan key says otherwise).
 * With ICIKT_FLAG_TIMING the keep, quantisation, permutation and class kernels are accounted under ICIKT_K_EPILOGUE.
 * icikt_permanova_in / icikt_permanova_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_PERMANOVA_MAX_CELLS (1ll << 26)
int icikt_permanova_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                        const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                        uint32_t flags, const int32_t *cls, int n_class, const int32_t *perm_cls, int64_t n_perm,
                        int64_t *n_pairs, int64_t *q_total, int64_t *bins_lo, int64_t *bins_hi, double *max_taumax,
                        int64_t *reason_counts);

/* ---- PERMDISP: every sample's sum of squared dissimilarities to every class -------------------------------------------
 *
 * The test that belongs beside PERMANOVA (Anderson & Walsh 2013): are the classes' dispersions homogeneous -- Anderson
 * 2006, vegan::betadisper(type = "centroid") with permutest -- on the dissimilarity 1 - raw.  The triangle runs as in
 * icikt_permanova_f64 and a pair's q is the same integer (csrc/icikt_fixed.h; a pair that is no value adds 0), so
 * n_pairs and q_total are bit for bit icikt_permanova_f64's on the same input.  This entry returns the table
 *   T[i][c] = sum of q_ij over the samples j != i with cls[j] = c      (0 for a class without a sample)
 * and nothing else: with n_c the class sizes and A_c = 1/2 sum_{i in c} T[i][c] (the within-class pairs' sum), the
 * squared distance of sample i to the centroid of class c in the full principal-coordinate space is
 *   D2(i, c) = (n_c T[i][c] - A_c) / (n_c^2 2^50),
 * a signed integer over a constant; the distances, their ANOVA F and the permutation test are the caller's, in integers
 * and rational arithmetic.
 *   cls, n_class   as icikt_class_matrix_f64 (a null cls: one class, n_class ignored); n_class <=
 *                  ICIKT_ANOSIM_MAX_CLASSES and n_samp n_class <= ICIKT_PERMDISP_MAX_CELLS (16 bytes per cell in the
 *                  caller's arrays, as many in the library's until the call has succeeded and on the device)
 *   n_pairs        [2] the values and the NA pairs
 *   q_total        [2] Q, the sum of q over all values: Q = q_total[1] 2^32 + q_total[0]
 *   t_lo, t_hi     [n_samp][n_class] row-major: T[i][c] = t_hi[i n_class + c] 2^32 + t_lo[i n_class + c].  THE LIMB RULE
 *                  of icikt_permanova_f64: 0 <= lo < 2^48 and 0 <= hi < 2^36 here; lo may exceed 2^32
 * AN NA PAIR adds 0 and the table is returned as summed; n_pairs[1] > 0 tells the caller that no centroid has a
 * meaning.  n_samp of 0 or 1 gives zero sums; it is no error.
 * All outputs but max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are required.  A bad n_class, a label
 * out of range, too many cells, a null output: ICIKT_E_INVALID before anything -- the context or an output -- is
 * touched.  n_samp <= ICIKT_TOPK_MAX_SAMPLES; n_feat, global_na and the state the call leaves behind (none): as
 * icikt_topk_f64.  The result is a pure function of the input, whatever the block cut or the grid.
 * Device memory: the prepared matrix, one block's buffers, 8 bytes per pair of the triangle for the kept keys
 * (n_samp = 65 535: 17 GB) and 16 n_samp n_class + 4 n_samp bytes of table and labels.
 * With ICIKT_FLAG_TIMING the keep and the table kernel are accounted under ICIKT_K_EPILOGUE.
 * icikt_permdisp_in / icikt_permdisp_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_PERMDISP_MAX_CELLS (1ll << 26)
int icikt_permdisp_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                       const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                       uint32_t flags, const int32_t *cls, int n_class, int64_t *n_pairs, int64_t *q_total,
                       int64_t *t_lo, int64_t *t_hi, double *max_taumax, int64_t *reason_counts);

/* ---- PCoA: the principal coordinates of the samples under 1 - raw -------------------------------------------------------
 *
 * The ordination every quality-control report draws first (classical scaling, Gower 1966; vegan::wcmdscale,
 * skbio.stats.ordination.pcoa) on the dissimilarity 1 - raw, without an S x S matrix on the host.  The triangle runs as
 * in icikt_permanova_f64 and a pair's q is the same integer (csrc/icikt_fixed.h), so n_pairs and q_total are bit for
 * bit icikt_permanova_f64's.  With e^_ij = q_ij 2^-50 (e^_ii = 0), the row sums R_i = sum_j q_ij and T = sum_i R_i = 2 Q
 * as integers, m_i = R_i / (S 2^50) and m-bar = T / (S^2 2^50) each one correctly rounded double, the centred table is
 *   G_ij = -0.5 * ((e^_ij - (m_i + m_j)) + m-bar)        (these four double operations, each rounded once)
 * and the call returns the k algebraically largest eigenvalues of G, descending, with orthonormal eigenvectors; a
 * vector's component of largest magnitude is positive (the smallest index among equal magnitudes decides).  The pairs
 * are found by a block Krylov iteration with full reorthogonalisation and Rayleigh-Ritz from the caller's start block;
 * every floating-point sum has a fixed order, so the result is a pure function of the input and the start block,
 * whatever the block cut, the call before or the stream.  The work is bounded: there is no restart.
 *   k            1 .. min(n_samp - 1, ICIKT_PCOA_MAX_K); n_samp >= 2
 *   tol          > 0: the iteration stops when every |G y - theta y|_2 <= tol |G|_F
 *   max_basis    the most basis columns; 0: min(n_samp, max(8 k, 128)); else >= k.  Capped at ICIKT_PCOA_MAX_BASIS and
 *                at n_samp; with max_basis = n_samp the basis spans the space and the call converges
 *   start        [k][n_samp]: column a of the start block is start[a n_samp + i]; finite, k independent columns
 *                (ICIKT_E_INVALID otherwise).  The library draws nothing itself
 *   n_pairs      [2] the values and the NA pairs
 *   q_total      [2] Q = q_total[1] 2^32 + q_total[0], the sum of q over all values
 *   row_lo, row_hi [n_samp]: R_i = row_hi[i] 2^32 + row_lo[i] (the limb rule of icikt_permanova_f64; lo may exceed 2^32)
 *   eigenvalues  [k]; vectors [k][n_samp]: component i of vector a is vectors[a n_samp + i]
 *   residuals    [k] |G y - theta y|_2 of the returned pairs; frobenius: |G|_F
 *   min_ritz     the smallest Ritz value of the last projected problem: an estimate (from above) of the most negative
 *                eigenvalue of G, which says how non-Euclidean the dissimilarity is
 *   solver       [3] n_basis: the basis columns used; n_apply: the applications of G to a block; converged: 1 or 0 (the
 *                basis filled up first: the best pairs so far are returned with the residuals as they are)
 *   gower        [n_samp][n_samp] G itself, or null: not returned
 * AN NA PAIR (n_pairs[1] > 0) makes every double -- eigenvalues, vectors, residuals, frobenius, min_ritz, gower -- R's
 * NA_real_ and solver zero; the integers are returned as summed.
 * All outputs but gower, max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are required.  A bad n_samp,
 * k, tol or max_basis, a null start block, a null output: ICIKT_E_INVALID before anything -- the context or an output --
 * is touched.  n_samp <= ICIKT_TOPK_MAX_SAMPLES; n_feat, global_na and the state the call leaves behind (none): as
 * icikt_topk_f64.
 * Device memory: the prepared matrix, one block's buffers, 8 bytes per pair of the triangle for the kept keys,
 * 8 n_samp^2 for G (n_samp = 65 535: 34 GB) and 16 n_samp max_basis + 8 n_samp (64 + 2 k) for the basis, its image,
 * a block and the Ritz vectors.  With ICIKT_FLAG_TIMING the keep and every kernel of the entry are accounted under
 * ICIKT_K_EPILOGUE.
 * icikt_pcoa_in / icikt_pcoa_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_PCOA_MAX_K 64
#define ICIKT_PCOA_MAX_BASIS 512
int icikt_pcoa_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld, const double *global_na,
                   int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int k, double tol,
                   int max_basis, const double *start, int64_t *n_pairs, int64_t *q_total, int64_t *row_lo,
                   int64_t *row_hi, double *eigenvalues, double *vectors, double *residuals, double *frobenius,
                   double *min_ritz, int64_t *solver, double *gower, double *max_taumax, int64_t *reason_counts);
/* The entry's hot kernel on DEVICE arrays, asynchronous on the context's stream (as icikt_convert_dev): d_W = d_G d_V
 * for a row-major n_samp x n_samp table d_G and blocks of 1 <= b <= ICIKT_PCOA_MAX_K columns, column c of a block at
 * [c n_samp, (c + 1) n_samp).  d_G is read once; every row's sum has a fixed order.  What tools/pcoa_time.py times and
 * tests/test_gpu_pcoa.py holds against numpy for every block width's code path. */
int icikt_pcoa_apply_dev(icikt_ctx *ctx, const double *d_G, const double *d_V, int64_t n_samp, int b, double *d_W);

/* ---- the Mantel test: 1 - raw against another matrix of the same samples, with its permutation test --------------------
 *
 * Mantel 1967; vegan::mantel, skbio.stats.distance.mantel.  The triangle runs as in icikt_anosim_f64; a pair is a VALUE
 * iff its raw is not NA.  x is the dissimilarity 1 - raw of the data matrix, y the caller's `other`: one finite double
 * per pair i < j in combn order (scipy's squareform order).  Both vectors become unsigned integers below 2^32:
 *   ICIKT_MANTEL_SPEARMAN   the doubled average rank among the P = n_samp (n_samp - 1) / 2 values, ascending in value:
 *                for x icikt_anosim_f64's r2 with M = P, for y lo + hi + 1 (lo: the values below, hi: those at or below)
 *   ICIKT_MANTEL_PEARSON    xv = llrint(ldexp(1.0 - raw, 30)), raw the double of the pair's key (-0 is +0), and
 *                yv = llrint(ldexp(y - lo, 31 - e)) with lo and hi the smallest and largest y, span = hi - lo and
 *                (m, e) = frexp(span): IEEE double, one rounding each, round half to even; both in 0 .. 2^31
 *                (csrc/icikt_mantel.h).  A span that is not finite is ICIKT_E_INVALID
 * For a permutation pi of the samples T(pi) = sum over i < j of xv_ij yv_{pi(i) pi(j)}; the observed T is that of the
 * identity.  With M = P: r = (M T - Sx Sy) / sqrt((M Sxx - Sx^2)(M Syy - Sy^2)), undefined when a factor is 0.  This
 * entry returns integers only; r is the caller's.
 *   other        [P] doubles, every one finite (one that is not: ICIKT_E_INVALID, the message names its position)
 *   perms        [n_perm][n_samp] row-major sample indices, 0 <= n_perm <= ICIKT_MANTEL_MAX_PERM; every row must be a
 *                permutation of 0 .. n_samp - 1 (else ICIKT_E_INVALID: "perms[q][s] = v occurs twice" / "is outside
 *                0 .. S - 1"); all rows are checked before anything is touched
 *   n_pairs      [2] the values and the NA pairs
 *   t_lo, t_hi   [1 + n_perm] T = t_hi 2^32 + t_lo, each limb a sum below 2^63 (t_lo may exceed 2^32); index 0 is the
 *                identity, index 1 + t permutation t
 *   moments      [8] Sx, Sxx, Sy, Syy as limbs: Sx = moments[1] 2^32 + moments[0], Sxx = moments[3] 2^32 + moments[2],
 *                Sy = moments[5] 2^32 + moments[4], Syy = moments[7] 2^32 + moments[6]
 *   n_ge, n_le   the permutations with T >= / <= the observed T, compared exactly as 128-bit integers: without an NA
 *                pair the denominator of r does not depend on the permutation.  (1 + n_ge) / (1 + n_perm) is vegan's
 *                p-value
 * WITH AN NA PAIR (n_pairs[1] > 0) nothing is summed: every T and moment is 0 and n_ge = n_le = 0; the permutations
 * are checked all the same.  n_samp of 0 or 1 gives zero sums; it is no error.
 * All outputs but max_taumax and reason_counts (as icikt_topk_f64, over all pairs) are required.  A bad method, a bad
 * n_perm, a null other or perms where one is needed, a null output, a value of other that is not finite, a row of perms
 * that is no permutation: ICIKT_E_INVALID before anything -- the context or an output -- is touched.  n_samp <=
 * ICIKT_TOPK_MAX_SAMPLES; n_feat, global_na and the state the call leaves behind (none): as icikt_topk_f64.  The result
 * is a pure function of the input, other and the permutations: integer sums, counts and comparisons, whatever the
 * block cut, the sort's tile, the batch, the strip or the grid.
 * Device memory: the prepared matrix, one block's buffers, 24 bytes per pair of the triangle (16 for pearson) for the
 * key planes, 4 n_samp^2 bytes for the table of y (n_samp = 65 535: 17 GB), and a batch of indices at two bytes each
 * (64 MB unless the anoperms plan key says otherwise).  A failed allocation is ICIKT_E_HIP.  With ICIKT_FLAG_TIMING
 * the kernels of y, the keep, the ranks or quantisation and the permutation kernel are accounted under
 * ICIKT_K_EPILOGUE.
 * icikt_mantel_in / icikt_mantel_csc: the same on a typed view / a CSC view of the matrix (below). */
#define ICIKT_MANTEL_MAX_PERM 1000000
#define ICIKT_MANTEL_PEARSON 0
#define ICIKT_MANTEL_SPEARMAN 1
int icikt_mantel_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld, const double *global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const double *other, int method, const int32_t *perms, int64_t n_perm, int64_t *n_pairs,
                     int64_t *t_lo, int64_t *t_hi, int64_t *moments, int64_t *n_ge, int64_t *n_le, double *max_taumax,
                     int64_t *reason_counts);

/* ---- query samples against a reference cohort: the query x reference rectangle ---------------------------------------
 *
 * Every column of Q (n_feat x n_query, leading dimension ld_query) with every column of R (n_feat x n_reference,
 * ld_reference): pair (q, r) is column q of Q with column r of R, and the call's pair order is query-major,
 * p = q n_reference + r.  No pair within Q or within R is computed.  global_na, perspective, alternative and continuity
 * apply to both matrices, as in icikt_matrix_f64.  A column that occurs in both matrices is a partner like any other.
 *   values       a pair's raw, pvalue, taumax and completeness are bit for bit what icikt_matrix_f64 reports for the same
 *                two columns of the stacked matrix [Q R] with the explicit pair list (q, n_query + r);
 *                cor = scale_max ? raw / max(taumax, na.rm = TRUE) : raw, the maximum over the RECTANGLE (-Inf when no
 *                pair has a taumax): what icikt_matrix_f64 scales by when that list is its pair list
 *   out5         (optional) [5][n_query][n_reference]: cor, raw, pvalue, taumax, completeness.  Device memory for the
 *                planes: 40 bytes per pair of the rectangle
 *   top-k        (optional: any of idx, out5k, n_valid; then 1 <= k <= ICIKT_TOPK_MAX) every query's k reference columns
 *                with the largest raw in icikt_topk_f64's strict order -- raw descending by the doubles' bits (-0.0 below
 *                +0.0), ties by the smaller reference index; a pair whose raw is NA is no partner.  idx [n_query][k]:
 *                reference column indices 0 .. n_reference - 1, -1 padded; out5k [5][n_query][k]: the five values,
 *                R's NA_real_ padded; n_valid [n_query]: real partners per query
 *   max_taumax   (optional) the scale's denominator; reason_counts (optional): [5] pairs of the rectangle per reason code
 * At least one output must be given.  n_query + n_reference, plus one when n_query is odd (the device matrix holds the
 * query columns, a padding column that makes the reference start on an even column, then the reference), is at most
 * ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID beyond, the message names the limit); n_feat as icikt_topk_f64 takes it.
 * n_query == 0 or n_reference == 0: an empty result (every list padding), no error.  Device memory beside the planes:
 * the prepared matrix of all columns, one block's buffers (whole query rows within the tkblock budget) and
 * 44 n_query k bytes of lists.  The state the call leaves behind (none) and the refusal of bad arguments before
 * anything -- the context or an output -- is touched: as icikt_topk_f64.  With ICIKT_FLAG_TIMING the folds are accounted
 * under ICIKT_K_EPILOGUE.
 * icikt_cross_in: the same on typed views of the two matrices (icikt_input, below), which may differ in element type
 * and order. */
int icikt_cross_f64(icikt_ctx *ctx, const double *Q, int64_t ld_query, const double *R, int64_t ld_reference,
                    int64_t n_feat, int64_t n_query, int64_t n_reference, const double *global_na, int n_global_na,
                    int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                    double *out5, int32_t *idx, double *out5k, int32_t *n_valid, double *max_taumax,
                    int64_t *reason_counts);
int icikt_cross_in(icikt_ctx *ctx, const icikt_input *Q, const icikt_input *R, int64_t n_feat, int64_t n_query,
                   int64_t n_reference, const double *global_na, int n_global_na, int k, int perspective,
                   int alternative, int continuity, uint32_t flags, int scale_max, double *out5, int32_t *idx,
                   double *out5k, int32_t *n_valid, double *max_taumax, int64_t *reason_counts);

/* ---- a reference cohort that stays prepared: batch after batch against the same reference ------------------------------
 *
 * icikt_cross_f64 uploads and pre-passes the reference with every call.  icikt_ref_prepare_f64 does that ONCE and leaves
 * the reference on the context; icikt_ref_cross_f64 then brings a batch of query columns alone and computes the same
 * rectangle, bit for bit.  The device matrix is the mirror of icikt_cross_f64's: the reference in columns
 * 0 .. n_reference - 1, one all-missing padding column when n_reference is odd, the batch from there on.
 *
 * icikt_ref_prepare_f64: R (n_feat x n_reference, leading dimension ld_reference), n_reference >= 1; global_na as
 * icikt_matrix_f64 takes it -- the rule is recorded and applies to every batch.  query_capacity >= 1 is the largest batch
 * the context will take: device memory for the reference and that many query columns is allocated here, once, and
 * never grows (0 is no way to say "unbounded": ICIKT_E_INVALID).  n_reference + query_capacity, plus one for each of
 * the two that is odd, is at most ICIKT_TOPK_MAX_SAMPLES (ICIKT_E_INVALID beyond, the message names the limit); n_feat
 * as icikt_topk_f64 takes it.  A second call replaces the reference.  icikt_run_dev answers ICIKT_E_STATE afterwards: the
 * prepared state is the reference's, not the device-resident calls'.
 * WHAT DROPS THE REFERENCE: every call that replaces the context's prepared state -- icikt_prepare_*, every host entry
 * that computes pairs or a missingness (icikt_pairs_*, icikt_matrix_*, icikt_pairs_complete_*, icikt_missingness_*,
 * the selection entries, icikt_cross_*), and an icikt_ref_cross_* that fails after its argument checks.  The next
 * icikt_ref_cross_* then returns ICIKT_E_STATE; it never reads tables another call has rewritten.  A caller that wants
 * the reference kept gives it a context of its own.
 *
 * icikt_ref_cross_f64: Q (n_feat x n_query, ld_query) against the prepared reference; n_feat must be the reference's and
 * n_query at most query_capacity (ICIKT_E_INVALID, the context and the reference stay as they are); no prepared
 * reference: ICIKT_E_STATE.  k, perspective ... scale_max, out5, idx, out5k, n_valid, max_taumax, reason_counts and
 * every refusal: as icikt_cross_f64, with n_reference the prepared one.  The call takes no global_na.
 *   ref_cls      (optional) [n_reference] a class index in 0 .. n_class - 1 per reference column, 1 <= n_class <= 65535;
 *                classes may be empty.  A class index outside the range is ICIKT_E_INVALID before anything is touched.
 *   cls_med2     (optional, needs ref_cls) [2][n_class][n_query], the query index fastest: med_cor and med_raw of cell
 *                (q, c).  The partners of the cell are the reference columns r of class c whose raw with q is not NA -- a
 *                column that occurs in both matrices is a partner like any other.  med_raw is R's median(raw, na.rm =
 *                TRUE) over them (a zero counts as +0; an even count: the correctly rounded mean of the two middle
 *                values); med_cor is the same rule on the cor cells of those one or two middle pairs (raw over the
 *                rectangle's largest taumax when scale_max, each quotient rounded first).  No partner: R's NA_real_
 *   cls_n_valid  (optional, needs ref_cls) [n_class][n_query] partners per cell
 * At least one output must be given.  n_query == 0: the empty result of icikt_cross_f64.  Device memory beside
 * icikt_cross_f64's: 20 n_query n_class bytes of cells and 4 n_reference bytes of member list (and 4 (n_class + 1)).
 * icikt_ref_info: the prepared reference's shape (any pointer may be null); ICIKT_E_STATE when there is none.
 * The _in twins: the same on a typed view of the matrix (icikt_input, below). */
int icikt_ref_prepare_f64(icikt_ctx *ctx, const double *R, int64_t ld_reference, int64_t n_feat, int64_t n_reference,
                          int64_t query_capacity, const double *global_na, int n_global_na, uint32_t flags);
int icikt_ref_prepare_in(icikt_ctx *ctx, const icikt_input *R, int64_t n_feat, int64_t n_reference,
                         int64_t query_capacity, const double *global_na, int n_global_na, uint32_t flags);
int icikt_ref_cross_f64(icikt_ctx *ctx, const double *Q, int64_t ld_query, int64_t n_feat, int64_t n_query, int k,
                        const int32_t *ref_cls, int n_class, int perspective, int alternative, int continuity,
                        uint32_t flags, int scale_max, double *out5, int32_t *idx, double *out5k, int32_t *n_valid,
                        double *cls_med2, int32_t *cls_n_valid, double *max_taumax, int64_t *reason_counts);
int icikt_ref_cross_in(icikt_ctx *ctx, const icikt_input *Q, int64_t n_feat, int64_t n_query, int k,
                       const int32_t *ref_cls, int n_class, int perspective, int alternative, int continuity,
                       uint32_t flags, int scale_max, double *out5, int32_t *idx, double *out5k, int32_t *n_valid,
                       double *cls_med2, int32_t *cls_n_valid, double *max_taumax, int64_t *reason_counts);
int icikt_ref_info(icikt_ctx *ctx, int64_t *n_feat, int64_t *n_reference, int64_t *query_capacity);

/* ---- several GPUs behind one call (what the R glue binds when n_gpu > 1) ----------------------
 *
 * Replaces the reference's worker fan-out, computation$split_fun(split_comparisons, ici_split, ...)
 * (R/kendalltau.R:158; chunks = ceiling(n_todo / ncore) consecutive pairs, :250-255; workers from
 * R/utils.R:68-80): one host thread per device inside ONE call from the R main thread.  Rank r uploads and
 * sorts its share of the columns only, the ranks all-gather the prepared columns (RCCL over xGMI), each runs
 * the pair kernel over block r of the pair list, and the results are gathered to the first device (RCCL) and
 * copied out once.  Same arguments, outputs and errors as icikt_pairs_f64. */
typedef struct icikt_multi icikt_multi;

#define ICIKT_MULTI_EXCHANGE_AUTO 0 /* RCCL when the listed devices are distinct, device copies otherwise */
#define ICIKT_MULTI_EXCHANGE_RCCL 1 /* ncclAllGather / ncclGather over xGMI */
#define ICIKT_MULTI_EXCHANGE_COPY 2 /* hipMemcpyPeerAsync between the ranks' buffers; a device may be listed
                                       more than once (how the flow is rehearsed on a one-GPU box) */
/* devices: n_gpu HIP device indices (NULL = 0 .. n_gpu-1).  Creates one context per entry and, for RCCL,
 * the communicators (ncclCommInitAll).  Keep the handle: creating communicators costs far more than a call. */
int icikt_multi_create(const int *devices, int n_gpu, int exchange, icikt_multi **out);
void icikt_multi_destroy(icikt_multi *m);
const char *icikt_multi_last_error(const icikt_multi *m);
int icikt_multi_n_gpu(const icikt_multi *m);
int icikt_multi_uses_rccl(const icikt_multi *m);
/* Ranks of the handle's RCCL communicator as RCCL reports them (ncclCommCount); 0 when the handle exchanges by device
 * copies and has no communicator, -1 on an RCCL error. */
int icikt_multi_comm_ranks(const icikt_multi *m);
int icikt_pairs_multi_f64(icikt_multi *m, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                          const int32_t *pi, const int32_t *pj, int64_t n_pairs, int perspective,
                          int alternative, int continuity, uint32_t flags, double *out4, int64_t *counts,
                          int32_t *reasons);
/* icikt_matrix_f64 on several GPUs: the ranks apply the exclusion rule to their own columns and return their rows
 * of `keep`; the first device assembles the five matrices from the gathered pair results and copies them out once. */
int icikt_matrix_multi_f64(icikt_multi *m, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                           const double *global_na, int n_global_na, const int32_t *pi, const int32_t *pj,
                           int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                           int scale_max, int diag_good, double *out5, uint8_t *keep, int64_t *reason_counts);
/* Wall-clock milliseconds of the last call's phases, the MAXIMUM over the ranks: H2D + pre-pass of the rank's
 * columns, exchange (all-gather + local rebuild), pair kernel + epilogue, gather + D2H.  With ICIKT_FLAG_TIMING each
 * phase ends with a stream synchronisation, so the figures are device time; without it they are host-side
 * enqueue times except the last, which absorbs everything still in flight.  The time a rank waits for the others
 * at the barriers between the phases is kept apart (icikt_multi_rank_phase_ms). */
#define ICIKT_MULTI_PHASE_PREPARE 0
#define ICIKT_MULTI_PHASE_EXCHANGE 1
#define ICIKT_MULTI_PHASE_PAIRS 2
#define ICIKT_MULTI_PHASE_GATHER 3
#define ICIKT_MULTI_PHASES 4
int icikt_multi_phase_ms(const icikt_multi *m, double *ms);
/* One rank's figures of the last call: ms[0 .. ICIKT_MULTI_PHASES-1] its phases, ms[ICIKT_MULTI_PHASES] the time it
 * waited for the other ranks at the barriers (ICIKT_MULTI_PHASES + 1 doubles): a spread between the ranks is
 * the imbalance of the partition. */
int icikt_multi_rank_phase_ms(const icikt_multi *m, int rank, double *ms);
/* Ranks the last icikt_pairs_multi_f64 call really used: n_gpu, or 1 when the job was too small to split (fewer
 * than two columns or 64 pairs per rank, no rows) or had wide columns (n_feat > ICIKT_MAX_FEATURES) and ran on the
 * first device alone; 0 after a call that failed its argument checks. */
int icikt_multi_ranks_used(const icikt_multi *m);
/* The cut of ICIKT_FLAG_BALANCE_COST as a function of its own (host arithmetic only, no device): col_cost[n_samp] = what
 * streaming each column costs; pj = the list's second indices (n_pairs of them), or n_pairs = -1 for all C(n_samp, 2)
 * pairs in combn order; n_blocks consecutive blocks of equal cost, none longer than max_block pairs (<= 0: no limit):
 * bounds[0 .. n_blocks], bounds[0] = 0, bounds[n_blocks] = the number of pairs. */
int icikt_cost_blocks(const uint32_t *col_cost, int64_t n_samp, const int32_t *pj, int64_t n_pairs, int n_blocks,
                      int64_t max_block, int64_t *bounds);
/* The pair blocks of the last call: rank r ran pairs [bounds[r], bounds[r + 1]) of the list (ranks_used + 1 values:
 * the reference's `core` chunks, or the cost-weighted cut of ICIKT_FLAG_BALANCE_COST). */
int icikt_multi_block_bounds(const icikt_multi *m, int64_t *bounds);
/* icikt_debug_set_plan() on every rank's context. */
int icikt_multi_debug_set_plan(icikt_multi *m, const char *spec);

/* kt_fast(use = "pairwise.complete.obs") (R/kendalltau.R:310-354, 448-545): for every pair the rows with a missing
 * value in EITHER vector are dropped, then ici_kt(..., perspective = "local") of what remains.  The masking, the
 * per-pair sorts and the counting all run on the device (pairs in chunks); same outputs as icikt_pairs_f64.
 * The call uses the context's prepared matrix and pair list for its own masked columns and leaves NEITHER behind,
 * whether it succeeds or fails: afterwards icikt_run_dev, icikt_expand_cols_dev and icikt_prep_arrays answer
 * ICIKT_E_STATE and icikt_num_pairs -1 until icikt_prepare_dev and icikt_set_pairs have been called again.  (A call
 * refused at its argument checks touches nothing.) */
int icikt_pairs_complete_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                             const int32_t *pi, const int32_t *pj, int64_t n_pairs, int alternative,
                             int continuity, uint32_t flags, double *out4, int64_t *counts, int32_t *reasons);

/* cor_fast (R/other_correlations.R): stats::cor.test estimates and p-values of Pearson or Spearman for every listed
 * pair of columns (self pairs allowed).  NaN = NA.  pairwise = 0: no NA in the listed columns (the caller has applied
 * use = "everything" / "complete.obs"); pairwise = 1: per pair, the rows missing in either column are dropped, and a
 * pair with fewer than 3 such rows is NA (cor_split).  alternative: ICIKT_ALT_TWO_SIDED / LESS / GREATER; continuity:
 * Spearman's t approximation only.  out3: P x 3 row-major (rho, p-value, n_values); reasons: ICIKT_COR_* per pair.
 * flags: ICIKT_FLAG_TIMING (icikt_kernel_ms: pre-pass, products, epilogue), ICIKT_FLAG_HOST_PINNED. */
#define ICIKT_METHOD_PEARSON 0
#define ICIKT_METHOD_SPEARMAN 1
#define ICIKT_COR_OK 0
#define ICIKT_COR_SHORT 1      /* too few rows: fewer than 3 (pairwise, Pearson) or 2 (Spearman): NA */
#define ICIKT_COR_NA 2         /* zero variance, or +-Inf in a Pearson pair: NA (cor's "standard deviation is zero") */
#define ICIKT_COR_TIES 3       /* Spearman, n < 1290 with ties: "Cannot compute exact p-value with ties", t approximation */
int icikt_cor_pairs_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                        const int32_t *pi, const int32_t *pj, int64_t n_pairs, int method, int pairwise,
                        int alternative, int continuity, uint32_t flags, double *out3, int32_t *reasons);

/* Missing-value diagnostics (R/left_censorship.R, R/rank-ordering.R).  X as everywhere: column-major
 * n_feat x n_samp, leading dimension ld.  A cell is missing when it is NaN or when setup_missing_matrix(global_na)
 * (R/utils.R:1-23) excludes it: global_na as in icikt_matrix_f64 (NaN = NA, +-Inf = Inf, at most 32 distinct finite
 * values, ICIKT_E_INVALID beyond: the front-ends mask such a matrix themselves and pass NaN).  n_feat up to
 * ICIKT_MAX_FEATURES_WIDE.  flags: ICIKT_FLAG_TIMING (icikt_kernel_ms: ICIKT_K_PREPARE the matrix's H2D, ICIKT_K_PAIRS
 * the column and row passes, ICIKT_K_EPILOGUE the gathers of rank_order), ICIKT_FLAG_HOST_PINNED.  NA results carry
 * R's NA_real_ bit pattern, NaN results R_NaN's (0x7FF8000000000000); a zero median is +0. */
/* medians[j]: stats::median of column j (calculate_matrix_medians(use = "col")); na_rm = 0: NA when the column has a
 * missing cell; NA for a column without values. */
int icikt_col_medians_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                          const double *global_na, int n_global_na, int na_rm, uint32_t flags, double *medians);
/* test_left_censorship's counts for every class at once: cls[j] in [0, n_class) is column j's class.  Per class, over the
 * rows with a missing cell among its columns: trials[k] = cells whose x < median(column, na.rm = TRUE) is not NA,
 * success[k] = cells where it is TRUE.  n_excluded: the cells the global_na rule excludes (the reference's early
 * return).  medians (optional, n_samp): the column medians the comparison used. */
int icikt_censor_counts_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                            const double *global_na, int n_global_na, const int32_t *cls, int n_class, uint32_t flags,
                            int64_t *trials, int64_t *success, int64_t *n_excluded, double *medians);
/* rank_order_data for one class, the columns cols[0 .. n_cols) (only they cross PCIe).  Rows missing in every listed
 * column are dropped; *n_kept rows stay.  Per row of X (n_feat): n_na = missing cells, median_rank = median of the row's
 * rank(x, na.last = FALSE) over the kept rows (NA_real_ for a dropped row).  row_order[0 .. n_kept): row indices of X,
 * order(median_rank, decreasing = TRUE) over the kept rows; col_order[n_cols]: positions in cols,
 * order(colMeans(is.na), decreasing = TRUE); both stable.  original / ordered (optional, n_kept x n_cols column-major,
 * room for n_feat x n_cols): the kept rows in row order / in row_order and col_order; missing cells NA_real_, the others
 * bitwise copies. */
int icikt_rank_order_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                         const double *global_na, int n_global_na, const int32_t *cols, int64_t n_cols, uint32_t flags,
                         int64_t *n_kept, int32_t *n_na, double *median_rank, int32_t *row_order, int32_t *col_order,
                         double *original, double *ordered);

/* pairwise_completeness() arithmetic (R/kendalltau.R:611-629): missingness[p] = #rows missing in
 * either column, from a host matrix whose missing cells are NaN.  Self pairs allowed. */
int icikt_missingness_f64(icikt_ctx *ctx, const double *X, int64_t n_feat, int64_t n_samp, int64_t ld,
                          const int32_t *pi, const int32_t *pj, int64_t n_pairs, int64_t *missingness);

/* ---- the host entries on a typed, strided view of the caller's matrix ------------------------------------------
 *
 * Each takes `const icikt_input *X, n_feat, n_samp` where its _f64 twin takes `const double *X, n_feat, n_samp, ld`;
 * every other argument, every output and the error contract are the twin's, and the _f64 entries are these with
 * {X, ICIKT_DTYPE_F64, ICIKT_ORDER_COL, ld}.  The matrix crosses PCIe in its own element type (float32 and int32:
 * half the bytes) and is widened / transposed on the device into the column-major float64 matrix the kernels read.
 * ICIKT_FLAG_HOST_PINNED keeps its meaning: the caller has page-locked `data`, which is then read in place.  A null
 * view or null data, an unknown dtype or order, ld below n_feat (COL) or n_samp (ROW): ICIKT_E_INVALID, the message
 * names the argument.  icikt_rank_order_in: consecutive columns are read in place in either order; other column lists
 * are gathered on the host, in the view's element type, before they cross PCIe. */
int icikt_pairs_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const int32_t *pi,
                   const int32_t *pj, int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                   double *out4, int64_t *counts, int32_t *reasons);
int icikt_topk_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                  int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  int32_t *idx, double *out5k, int32_t *n_valid, double *max_taumax, int64_t *reason_counts);
int icikt_edges_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                   int n_global_na, const icikt_edge_rule *rule, int perspective, int alternative, int continuity,
                   uint32_t flags, int scale_max, int64_t max_edges, int32_t *ei, int32_t *ej, double *out5e,
                   int64_t *n_edges, int64_t *degree, double *max_taumax, int64_t *reason_counts);
int icikt_class_medians_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                           int n_global_na, const int32_t *cls, int n_class, int perspective, int alternative,
                           int continuity, uint32_t flags, int scale_max, double *med2, int32_t *n_valid,
                           double *max_taumax, int64_t *reason_counts);
int icikt_quantiles_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                       int n_global_na, const int32_t *cls, int n_class, int perspective, int alternative,
                       int continuity, uint32_t flags, int scale_max, const double *probs, int n_probs,
                       const double *breaks, int n_breaks, double *q2, double *order2, int64_t *n_valid, int64_t *n_na,
                       int64_t *hist, int64_t *outside, double *max_taumax, int64_t *reason_counts);
int icikt_class_matrix_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                          int n_global_na, const int32_t *cls, int n_class, int perspective, int alternative,
                          int continuity, uint32_t flags, int scale_max, double *med2, int32_t *n_valid,
                          double *max_taumax, int64_t *reason_counts);
int icikt_padjust_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int method,
                     const double *alpha, int n_alpha, int64_t max_table, int64_t *n_tests, int64_t *n_rejected,
                     double *p_cutoff, double *table, int64_t *n_table, double *max_taumax, int64_t *reason_counts);
int icikt_mst_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                 int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                 double min_raw, int32_t *ti, int32_t *tj, double *out5t, int64_t *n_tree, int32_t *component,
                 int64_t *n_components, int32_t *n_rounds, double *max_taumax, int64_t *reason_counts);
int icikt_hclust_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                    int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                    int method, double min_raw, int32_t *ma, int32_t *mb, int32_t *msize, double *mraw, double *mcor,
                    int64_t *n_merges, int32_t *component, int64_t *n_components, double *max_taumax,
                    int64_t *reason_counts);
int icikt_anosim_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                    int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                    const int32_t *cls, int n_class, const int32_t *perm_cls, int64_t n_perm, int64_t *n_pairs,
                    int64_t *w2, int64_t *nw, int64_t *n_ge, int64_t *n_undefined, int64_t *class_w2,
                    int64_t *class_nw, double *max_taumax, int64_t *reason_counts);
int icikt_permanova_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                       int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                       const int32_t *cls, int n_class, const int32_t *perm_cls, int64_t n_perm, int64_t *n_pairs,
                       int64_t *q_total, int64_t *bins_lo, int64_t *bins_hi, double *max_taumax,
                       int64_t *reason_counts);
int icikt_permdisp_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                      int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                      const int32_t *cls, int n_class, int64_t *n_pairs, int64_t *q_total, int64_t *t_lo,
                      int64_t *t_hi, double *max_taumax, int64_t *reason_counts);
int icikt_pcoa_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                  int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int k, double tol,
                  int max_basis, const double *start, int64_t *n_pairs, int64_t *q_total, int64_t *row_lo,
                  int64_t *row_hi, double *eigenvalues, double *vectors, double *residuals, double *frobenius,
                  double *min_ritz, int64_t *solver, double *gower, double *max_taumax, int64_t *reason_counts);
int icikt_mantel_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const double *other, int method, const int32_t *perms, int64_t n_perm, int64_t *n_pairs,
                     int64_t *t_lo, int64_t *t_hi, int64_t *moments, int64_t *n_ge, int64_t *n_le, double *max_taumax,
                     int64_t *reason_counts);
int icikt_matrix_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                    int n_global_na, const int32_t *pi, const int32_t *pj, int64_t n_pairs, int perspective,
                    int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double *out5,
                    uint8_t *keep, int64_t *reason_counts);
int icikt_pairs_complete_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const int32_t *pi,
                            const int32_t *pj, int64_t n_pairs, int alternative, int continuity, uint32_t flags,
                            double *out4, int64_t *counts, int32_t *reasons);
int icikt_missingness_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const int32_t *pi,
                         const int32_t *pj, int64_t n_pairs, int64_t *missingness);
int icikt_cor_pairs_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const int32_t *pi,
                       const int32_t *pj, int64_t n_pairs, int method, int pairwise, int alternative, int continuity,
                       uint32_t flags, double *out3, int32_t *reasons);
int icikt_col_medians_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                         int n_global_na, int na_rm, uint32_t flags, double *medians);
int icikt_censor_counts_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp,
                           const double *global_na, int n_global_na, const int32_t *cls, int n_class, uint32_t flags,
                           int64_t *trials, int64_t *success, int64_t *n_excluded, double *medians);
int icikt_rank_order_in(icikt_ctx *ctx, const icikt_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                        int n_global_na, const int32_t *cols, int64_t n_cols, uint32_t flags, int64_t *n_kept,
                        int32_t *n_na, double *median_rank, int32_t *row_order, int32_t *col_order, double *original,
                        double *ordered);
/* The conversion alone, device to device, asynchronous on the context's stream: d_src is a DEVICE block of `dtype` cells
 * in `order` with leading dimension ld (elements); d_dst receives the column-major float64 matrix with leading dimension
 * dst_ld >= n_feat (rows [n_feat, dst_ld) of d_dst are left as they are) -- what icikt_prepare_dev takes.  The way in
 * for a matrix that is on the device already (a torch tensor's data_ptr()).  The two blocks must not overlap. */
int icikt_convert_dev(icikt_ctx *ctx, const void *d_src, int dtype, int order, int64_t n_feat, int64_t n_samp,
                      int64_t ld, double *d_dst, int64_t dst_ld);

/* ---- the host entries on a compressed-sparse-column view (icikt_csc_input above) ----------------------------------
 *
 * Each takes `const icikt_csc_input *X, n_feat, n_samp` where its _in twin takes `const icikt_input *X, n_feat, n_samp`;
 * every other argument, every output and the error contract are the twin's, plus the argument errors of a malformed
 * view.  The chunks, the pre-pass and the pair-kernel launches are the ones the dense float64 matrix would run; only
 * values[e0:e1] and indices[e0:e1] of a chunk's columns cross PCIe (8 d n S + 4 (S + 1) bytes for float32 values and
 * int32 indices at density d, where the dense float32 matrix moves 4 n S).  ICIKT_FLAG_HOST_PINNED keeps its meaning: the
 * caller has page-locked `values`, `indices` and the result arrays; indptr is read by the host and copied once.
 * icikt_rank_order_csc: consecutive columns are read in place; any other column list is gathered on the host as slices
 * of values / indices plus a rebuilt indptr, O(entries of the listed columns). */
int icikt_pairs_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const int32_t *pi,
                    const int32_t *pj, int64_t n_pairs, int perspective, int alternative, int continuity, uint32_t flags,
                    double *out4, int64_t *counts, int32_t *reasons);
int icikt_matrix_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                     int n_global_na, const int32_t *pi, const int32_t *pj, int64_t n_pairs, int perspective,
                     int alternative, int continuity, uint32_t flags, int scale_max, int diag_good, double *out5,
                     uint8_t *keep, int64_t *reason_counts);
int icikt_topk_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                   int n_global_na, int k, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                   int32_t *idx, double *out5k, int32_t *n_valid, double *max_taumax, int64_t *reason_counts);
int icikt_edges_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                    int n_global_na, const icikt_edge_rule *rule, int perspective, int alternative, int continuity,
                    uint32_t flags, int scale_max, int64_t max_edges, int32_t *ei, int32_t *ej, double *out5e,
                    int64_t *n_edges, int64_t *degree, double *max_taumax, int64_t *reason_counts);
int icikt_class_medians_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                            const double *global_na, int n_global_na, const int32_t *cls, int n_class, int perspective,
                            int alternative, int continuity, uint32_t flags, int scale_max, double *med2,
                            int32_t *n_valid, double *max_taumax, int64_t *reason_counts);
int icikt_quantiles_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                        int n_global_na, const int32_t *cls, int n_class, int perspective, int alternative,
                        int continuity, uint32_t flags, int scale_max, const double *probs, int n_probs,
                        const double *breaks, int n_breaks, double *q2, double *order2, int64_t *n_valid, int64_t *n_na,
                        int64_t *hist, int64_t *outside, double *max_taumax, int64_t *reason_counts);
int icikt_class_matrix_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                           const double *global_na, int n_global_na, const int32_t *cls, int n_class, int perspective,
                           int alternative, int continuity, uint32_t flags, int scale_max, double *med2,
                           int32_t *n_valid, double *max_taumax, int64_t *reason_counts);
int icikt_padjust_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                      int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int method,
                      const double *alpha, int n_alpha, int64_t max_table, int64_t *n_tests, int64_t *n_rejected,
                      double *p_cutoff, double *table, int64_t *n_table, double *max_taumax, int64_t *reason_counts);
int icikt_mst_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                  int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                  double min_raw, int32_t *ti, int32_t *tj, double *out5t, int64_t *n_tree, int32_t *component,
                  int64_t *n_components, int32_t *n_rounds, double *max_taumax, int64_t *reason_counts);
int icikt_hclust_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int scale_max,
                     int method, double min_raw, int32_t *ma, int32_t *mb, int32_t *msize, double *mraw, double *mcor,
                     int64_t *n_merges, int32_t *component, int64_t *n_components, double *max_taumax,
                     int64_t *reason_counts);
int icikt_anosim_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const int32_t *cls, int n_class, const int32_t *perm_cls, int64_t n_perm, int64_t *n_pairs,
                     int64_t *w2, int64_t *nw, int64_t *n_ge, int64_t *n_undefined, int64_t *class_w2,
                     int64_t *class_nw, double *max_taumax, int64_t *reason_counts);
int icikt_permanova_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                        const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                        uint32_t flags, const int32_t *cls, int n_class, const int32_t *perm_cls, int64_t n_perm,
                        int64_t *n_pairs, int64_t *q_total, int64_t *bins_lo, int64_t *bins_hi, double *max_taumax,
                        int64_t *reason_counts);
int icikt_permdisp_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                       const double *global_na, int n_global_na, int perspective, int alternative, int continuity,
                       uint32_t flags, const int32_t *cls, int n_class, int64_t *n_pairs, int64_t *q_total,
                       int64_t *t_lo, int64_t *t_hi, double *max_taumax, int64_t *reason_counts);
int icikt_pcoa_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                   int n_global_na, int perspective, int alternative, int continuity, uint32_t flags, int k, double tol,
                   int max_basis, const double *start, int64_t *n_pairs, int64_t *q_total, int64_t *row_lo,
                   int64_t *row_hi, double *eigenvalues, double *vectors, double *residuals, double *frobenius,
                   double *min_ritz, int64_t *solver, double *gower, double *max_taumax, int64_t *reason_counts);
int icikt_mantel_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const double *global_na,
                     int n_global_na, int perspective, int alternative, int continuity, uint32_t flags,
                     const double *other, int method, const int32_t *perms, int64_t n_perm, int64_t *n_pairs,
                     int64_t *t_lo, int64_t *t_hi, int64_t *moments, int64_t *n_ge, int64_t *n_le, double *max_taumax,
                     int64_t *reason_counts);
int icikt_missingness_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp, const int32_t *pi,
                          const int32_t *pj, int64_t n_pairs, int64_t *missingness);
int icikt_col_medians_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                          const double *global_na, int n_global_na, int na_rm, uint32_t flags, double *medians);
int icikt_censor_counts_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                            const double *global_na, int n_global_na, const int32_t *cls, int n_class, uint32_t flags,
                            int64_t *trials, int64_t *success, int64_t *n_excluded, double *medians);
int icikt_rank_order_csc(icikt_ctx *ctx, const icikt_csc_input *X, int64_t n_feat, int64_t n_samp,
                         const double *global_na, int n_global_na, const int32_t *cols, int64_t n_cols, uint32_t flags,
                         int64_t *n_kept, int32_t *n_na, double *median_rank, int32_t *row_order, int32_t *col_order,
                         double *original, double *ordered);
/* The scatter alone, for arrays that are on the device already (the counterpart of icikt_convert_dev): d_values,
 * d_indices and d_indptr are DEVICE arrays of a CSC matrix as in icikt_csc_input; d_dst receives the column-major
 * float64 matrix with leading dimension dst_ld >= n_feat (rows [n_feat, dst_ld) of d_dst are left as they are).
 * Unlike icikt_convert_dev it RETURNS AFTER THE CONTEXT'S STREAM HAS BEEN SYNCHRONISED, so that it can report malformed
 * input: indptr is read back and checked as the host entries check it, the entries are checked by the kernel. */
int icikt_scatter_csc_dev(icikt_ctx *ctx, const void *d_values, const void *d_indices, const void *d_indptr, int dtype,
                          int index_type, double fill, int64_t n_feat, int64_t n_samp, double *d_dst, int64_t dst_ld);

/* Device self-test of the wavefront primitives the pair kernel relies on (DPP scan / shift). */
int icikt_selftest(icikt_ctx *ctx);

/* Development / test hook (the product path reads no environment variable): "key=value,key=value" overrides of
 * the pair kernel's launch plan and of the host path's H2D mode on this context; NULL or "" restores the library's
 * choices.  Keys: np (pairs per wave: 1 | 2), pend (l | g: open-group bitset in LDS | global memory), wpb (waves
 * per workgroup), half (0 | 1), tgmax (joint ties of long tie groups by the gathered column's tie groups -- list or count
 * mode -- up to this many of them; -1 = per-row mode), list (list mode up to this many tie groups, <= 128: count mode
 * takes over above), solo (0: SOLO steps run as MIXED steps), waves (half-wave kernels: waves per CU down to which the
 * pairs' counter tables may cost the launch occupancy), split (1 | 2 | 4: segments a half-wave task is cut in, whatever the
 * launch's size), merge (0 | 1: the pipelined host entries' pairs in a launch per chunk | in one launch behind the last chunk), gridmult / gridcap (persistent grid of the long-column kernel: a
 * multiple of the resident workgroups / at most this many), pipe (0 | 1: the host entries' chunk pipeline), k0 (0 | 1: the
 * pre-pass always in its 1 024-thread / 256-thread shape), tkblock (icikt_topk_* and icikt_edges_*: the pairs a block of whole combn rows
 * may hold -- a block is always at least one row, so tkblock=1 runs a row per block; icikt_class_medians_*: the same
 * budget for the rows of one class and for the slices of several classes' pair list), medlds (icikt_class_medians_*:
 * the partners up to which the select kernel gathers a sample's keys into LDS once, 0 .. 4096; a sample with more
 * re-reads the kept plane in every pass), qbatch (icikt_quantiles_*: the targets -- distinct (group, rank) -- the
 * select runs per batch of eight passes, 1 .. 32), padjtile (icikt_padjust_*: the keys of a tile of the sort, the run one
 * wave counts and scatters in order, 1 .. 2^30; raised when the plane would have more than 65 536 tiles; icikt_anosim_* sorts with
 * the same tile), anoperms (icikt_anosim_*: the labellings per upload, 1 .. 2^20; the permutation kernel takes them 16 at a
 * time), anostrip (icikt_anosim_*: the columns of the triangle a workgroup of the permutation kernel owns, 1 .. 4096; anoperms and anostrip
 * apply to icikt_permanova_* as well), hcgrid (icikt_hclust_*: the workgroups of the
 * kernel that rescans the listed rows of a step, 1 .. 256; default min(n_samp, 256)), verbose (0 | 1: print the chosen
 * plan to stderr). */
int icikt_debug_set_plan(icikt_ctx *ctx, const char *spec);
/* Development hook: per step kind of the pair kernel (hot loop, hot step in the main loop, MIXED, GROUP, general,
 * closed-form tail, set-up) the steps taken, their rows and the wave cycles spent, as out24 = [steps x 8 | rows x 8 |
 * cycles x 8] since the last reset.  Counted only by a diagnostic build of the library (-DICIKT_STEP_STATS,
 * tools/step_stats.py); the product build executes no stamp and answers ICIKT_E_STATE. */
int icikt_debug_step_stats(icikt_ctx *ctx, uint64_t *out24, int reset);

#ifdef __cplusplus
}
#endif
#endif /* ICIKT_H */
