/*
 * icikt_rglue_diag.c -- R .Call glue of the missing-value diagnostics (R/left_censorship.R, R/rank-ordering.R) over
 * icikt_col_medians_f64, icikt_censor_counts_f64 and icikt_rank_order_f64 (include/icikt.h).
 *
 * A DLL of its own beside icikt_rglue.c and icikt_rglue_cor.c (whose registered tables stay as they are):
 *
 *   R CMD SHLIB -o icikt_rglue_diag.so icikt_rglue_diag.c -I<repo>/include -L<repo>/icikendalltau_amd -licikt_hip
 *
 * Registered routines (x: REALSXP matrix n x S, column-major; global_na: REALSXP, NA / Inf / finite values, at most 32
 * distinct finite ones -- the R wrappers mask a longer list themselves and pass NA):
 *   .Call("icikt_R_col_medians", x, global_na, na_rm, device)     -> REALSXP medians of the columns
 *   .Call("icikt_R_censor_counts", x, global_na, cls, device)
 *       cls  INTSXP (the wrapper passes as.integer()), 1-based class of every column (as.integer(factor(sample_classes))),
 *            classes 1 .. max(cls)
 *       returns list(trials, success, n_excluded) (doubles; trials / success per class)
 *   .Call("icikt_R_rank_order", x, global_na, cols, device)
 *       cols INTSXP, 1-based columns of the class
 *       returns list(n_na, median_rank, row_order, col_order, original, ordered): n_na / median_rank over the kept rows,
 *       row_order 1-based rows of x, col_order 1-based positions in cols, original / ordered n_kept x length(cols)
 * Errors become R errors (Rf_error).
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <string.h>

#include "icikt.h"

static icikt_ctx *g_diag_ctx = NULL;
static int g_diag_dev = -1;

static icikt_ctx *diag_ctx(int device) {
  if (g_diag_ctx && g_diag_dev == device) return g_diag_ctx;
  if (g_diag_ctx) { icikt_ctx_destroy(g_diag_ctx); g_diag_ctx = NULL; }
  int rc = icikt_ctx_create(device, &g_diag_ctx);
  if (rc == ICIKT_E_NO_DEVICE) Rf_error("icikt: no usable HIP device (there is no CPU fallback)");
  if (rc != ICIKT_SUCCESS) Rf_error("icikt: icikt_ctx_create(%d) failed with code %d", device, rc);
  g_diag_dev = device;
  return g_diag_ctx;
}

static void check_matrix(SEXP x) {
  if (!Rf_isReal(x) || !Rf_isMatrix(x)) Rf_error("icikt: x must be a double matrix");
}

static void check_global_na(SEXP global_na) {
  if (!Rf_isReal(global_na) && !Rf_isNull(global_na)) Rf_error("icikt: global_na must be a double vector");
}

static const double *gna_ptr(SEXP global_na) { return Rf_isNull(global_na) ? NULL : REAL(global_na); }
static int gna_len(SEXP global_na) { return Rf_isNull(global_na) ? 0 : (int)XLENGTH(global_na); }

SEXP icikt_R_col_medians(SEXP x, SEXP global_na, SEXP na_rm, SEXP device) {
  check_matrix(x);
  check_global_na(global_na);
  const int64_t n = Rf_nrows(x), S = Rf_ncols(x);
  icikt_ctx *ctx = diag_ctx(Rf_asInteger(device));
  SEXP res = PROTECT(Rf_allocVector(REALSXP, S));
  int rc = icikt_col_medians_f64(ctx, REAL(x), n, S, n > 0 ? n : 1, gna_ptr(global_na), gna_len(global_na),
                                 Rf_asLogical(na_rm) == TRUE, 0u,
                                 REAL(res));
  if (rc != ICIKT_SUCCESS) Rf_error("icikt: %s (code %d)", icikt_last_error(ctx), rc);
  UNPROTECT(1);
  return res;
}

SEXP icikt_R_censor_counts(SEXP x, SEXP global_na, SEXP cls, SEXP device) {
  check_matrix(x);
  check_global_na(global_na);
  const int64_t n = Rf_nrows(x), S = Rf_ncols(x);
  if (XLENGTH(cls) != S || S < 1) Rf_error("icikt: cls must give one class per column");
  int nc = 1;
  for (int64_t j = 0; j < S; ++j) nc = INTEGER(cls)[j] > nc ? INTEGER(cls)[j] : nc;
  int32_t *cls0 = (int32_t *)R_alloc(S > 0 ? S : 1, sizeof(int32_t));
  for (int64_t j = 0; j < S; ++j) {
    const int k = INTEGER(cls)[j];
    if (k < 1 || k > nc) Rf_error("icikt: class index out of range");
    cls0[j] = k - 1;
  }
  icikt_ctx *ctx = diag_ctx(Rf_asInteger(device));
  int64_t *tr = (int64_t *)R_alloc(nc, sizeof(int64_t)), *su = (int64_t *)R_alloc(nc, sizeof(int64_t)), nex = 0;
  int rc = icikt_censor_counts_f64(ctx, REAL(x), n, S, n > 0 ? n : 1, gna_ptr(global_na), gna_len(global_na), cls0, nc,
                                   0u, tr, su, &nex, NULL);
  if (rc != ICIKT_SUCCESS) Rf_error("icikt: %s (code %d)", icikt_last_error(ctx), rc);
  const char *nm[] = {"trials", "success", "n_excluded", ""};
  SEXP res = PROTECT(Rf_mkNamed(VECSXP, nm));
  SEXP t = PROTECT(Rf_allocVector(REALSXP, nc)), s = PROTECT(Rf_allocVector(REALSXP, nc));
  for (int k = 0; k < nc; ++k) { REAL(t)[k] = (double)tr[k]; REAL(s)[k] = (double)su[k]; }
  SEXP e = PROTECT(Rf_allocVector(REALSXP, 1));
  REAL(e)[0] = (double)nex;
  SET_VECTOR_ELT(res, 0, t);
  SET_VECTOR_ELT(res, 1, s);
  SET_VECTOR_ELT(res, 2, e);
  UNPROTECT(4);
  return res;
}

SEXP icikt_R_rank_order(SEXP x, SEXP global_na, SEXP cols, SEXP device) {
  check_matrix(x);
  check_global_na(global_na);
  const int64_t n = Rf_nrows(x), S = Rf_ncols(x), m = XLENGTH(cols);
  if (m < 1) Rf_error("icikt: cols must not be empty");
  int32_t *cols0 = (int32_t *)R_alloc(m, sizeof(int32_t));
  for (int64_t j = 0; j < m; ++j) {
    cols0[j] = INTEGER(cols)[j] - 1;
    if (cols0[j] < 0 || cols0[j] >= S) Rf_error("icikt: column index out of range");
  }
  icikt_ctx *ctx = diag_ctx(Rf_asInteger(device));
  const size_t nn = n > 0 ? (size_t)n : 1;
  int32_t *n_na = (int32_t *)R_alloc(nn, sizeof(int32_t)), *rord = (int32_t *)R_alloc(nn, sizeof(int32_t));
  int32_t *cord = (int32_t *)R_alloc(m, sizeof(int32_t));
  double *med = (double *)R_alloc(nn, sizeof(double));
  double *orig = (double *)R_alloc(nn * (size_t)m, sizeof(double)), *ordd = (double *)R_alloc(nn * (size_t)m, sizeof(double));
  int64_t nk = 0;
  int rc = icikt_rank_order_f64(ctx, REAL(x), n, S, n > 0 ? n : 1, gna_ptr(global_na), gna_len(global_na), cols0, m, 0u,
                                &nk, n_na, med, rord, cord, orig, ordd);
  if (rc != ICIKT_SUCCESS) Rf_error("icikt: %s (code %d)", icikt_last_error(ctx), rc);
  const char *nm[] = {"n_na", "median_rank", "row_order", "col_order", "original", "ordered", ""};
  SEXP res = PROTECT(Rf_mkNamed(VECSXP, nm));
  SEXP v_na = PROTECT(Rf_allocVector(INTSXP, nk)), v_med = PROTECT(Rf_allocVector(REALSXP, nk));
  SEXP v_ro = PROTECT(Rf_allocVector(INTSXP, nk)), v_co = PROTECT(Rf_allocVector(INTSXP, m));
  int64_t i = 0;
  for (int64_t r = 0; r < n; ++r)
    if (n_na[r] < m) { INTEGER(v_na)[i] = n_na[r]; REAL(v_med)[i] = med[r]; ++i; }
  for (int64_t k = 0; k < nk; ++k) INTEGER(v_ro)[k] = rord[k] + 1;
  for (int64_t j = 0; j < m; ++j) INTEGER(v_co)[j] = cord[j] + 1;
  SEXP v_or = PROTECT(Rf_allocMatrix(REALSXP, (int)nk, (int)m)), v_od = PROTECT(Rf_allocMatrix(REALSXP, (int)nk, (int)m));
  if (nk > 0) {
    memcpy(REAL(v_or), orig, (size_t)nk * (size_t)m * sizeof(double));
    memcpy(REAL(v_od), ordd, (size_t)nk * (size_t)m * sizeof(double));
  }
  SET_VECTOR_ELT(res, 0, v_na);
  SET_VECTOR_ELT(res, 1, v_med);
  SET_VECTOR_ELT(res, 2, v_ro);
  SET_VECTOR_ELT(res, 3, v_co);
  SET_VECTOR_ELT(res, 4, v_or);
  SET_VECTOR_ELT(res, 5, v_od);
  UNPROTECT(7);
  return res;
}

static const R_CallMethodDef CallEntries[] = {
    {"icikt_R_col_medians", (DL_FUNC)&icikt_R_col_medians, 4},
    {"icikt_R_censor_counts", (DL_FUNC)&icikt_R_censor_counts, 4},
    {"icikt_R_rank_order", (DL_FUNC)&icikt_R_rank_order, 4},
    {NULL, NULL, 0}};

void R_init_icikt_rglue_diag(DllInfo *dll) {
  R_registerRoutines(dll, NULL, CallEntries, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}

void R_unload_icikt_rglue_diag(DllInfo *dll) {
  (void)dll;
  if (g_diag_ctx) { icikt_ctx_destroy(g_diag_ctx); g_diag_ctx = NULL; }
}
