/*
 * icikt_rglue_cor.c -- R .Call glue of cor_fast (R/other_correlations.R) over icikt_cor_pairs_f64 (include/icikt.h).
 *
 * A DLL of its own beside icikt_rglue.c (whose registered table stays as it is):
 *
 *   R CMD SHLIB -o icikt_rglue_cor.so icikt_rglue_cor.c -I<repo>/include -L<repo>/icikendalltau_amd -licikt_hip
 *
 * Registered routine:
 *   .Call("icikt_R_cor", x, pi, pj, method, pairwise, alternative, continuity, device, timing)
 *       x            REALSXP matrix n x S (column-major, NA = missing); with pairwise = FALSE it must hold no NA (the R
 *                    wrapper applies use = "everything" / "complete.obs" first, as cor_fast does)
 *       pi, pj       INTSXP, 1-based column indices of the pairs (setup_comparisons(diag_good = FALSE) order)
 *       method       "pearson" | "spearman";  alternative  "two.sided" | "less" | "greater"
 *       timing       TRUE: also kernel_ms = c(prepare, products, epilogue) of this call
 *       returns list(rho, pvalue, n_values, reason[, kernel_ms]) of length-P vectors; reason: ICIKT_COR_* per pair
 * Errors become R errors (Rf_error).
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <string.h>

#include "icikt.h"

/* R's NA_real_: a NaN with payload 1954 (what is.na() and print() tell apart from NaN) */
static double na_real(void) {
  const uint64_t bits = 0x7FF00000000007A2ull;
  double d;
  memcpy(&d, &bits, sizeof d);
  return d;
}

static icikt_ctx *g_cor_ctx = NULL;
static int g_cor_dev = -1;

static icikt_ctx *cor_ctx(int device) {
  if (g_cor_ctx && g_cor_dev == device) return g_cor_ctx;
  if (g_cor_ctx) { icikt_ctx_destroy(g_cor_ctx); g_cor_ctx = NULL; }
  int rc = icikt_ctx_create(device, &g_cor_ctx);
  if (rc == ICIKT_E_NO_DEVICE) Rf_error("icikt: no usable HIP device (there is no CPU fallback)");
  if (rc != ICIKT_SUCCESS) Rf_error("icikt: icikt_ctx_create(%d) failed with code %d", device, rc);
  g_cor_dev = device;
  return g_cor_ctx;
}

SEXP icikt_R_cor(SEXP x, SEXP pi, SEXP pj, SEXP method, SEXP pairwise, SEXP alternative, SEXP continuity,
                 SEXP device, SEXP timing) {
  if (!Rf_isReal(x) || !Rf_isMatrix(x)) Rf_error("icikt: x must be a double matrix");
  const char *m = CHAR(STRING_ELT(method, 0)), *a = CHAR(STRING_ELT(alternative, 0));
  int meth, alt;
  if (strcmp(m, "pearson") == 0) meth = ICIKT_METHOD_PEARSON;
  else if (strcmp(m, "spearman") == 0) meth = ICIKT_METHOD_SPEARMAN;
  else Rf_error("icikt: method must be \"pearson\" or \"spearman\"");
  if (strcmp(a, "two.sided") == 0) alt = ICIKT_ALT_TWO_SIDED;
  else if (strcmp(a, "less") == 0) alt = ICIKT_ALT_LESS;
  else if (strcmp(a, "greater") == 0) alt = ICIKT_ALT_GREATER;
  else Rf_error("icikt: alternative must be \"two.sided\", \"less\" or \"greater\"");
  const int64_t n_feat = Rf_nrows(x), n_samp = Rf_ncols(x), P = XLENGTH(pi);
  if (XLENGTH(pj) != P) Rf_error("icikt: pi and pj differ in length");
  const int with_timing = Rf_asLogical(timing) == TRUE;
  icikt_ctx *ctx = cor_ctx(Rf_asInteger(device));
  int32_t *pi0 = (int32_t *)R_alloc(P > 0 ? P : 1, sizeof(int32_t));
  int32_t *pj0 = (int32_t *)R_alloc(P > 0 ? P : 1, sizeof(int32_t));
  for (int64_t p = 0; p < P; ++p) { pi0[p] = INTEGER(pi)[p] - 1; pj0[p] = INTEGER(pj)[p] - 1; }
  double *out3 = (double *)R_alloc((size_t)(P > 0 ? 3 * P : 1), sizeof(double));
  int32_t *reasons = (int32_t *)R_alloc(P > 0 ? P : 1, sizeof(int32_t));
  if (with_timing) icikt_reset_timers(ctx);
  int rc = icikt_cor_pairs_f64(ctx, REAL(x), n_feat, n_samp, n_feat, pi0, pj0, P, meth, Rf_asLogical(pairwise) == TRUE,
                               alt, Rf_asLogical(continuity) == TRUE, with_timing ? ICIKT_FLAG_TIMING : 0u, out3, reasons);
  if (rc != ICIKT_SUCCESS) Rf_error("icikt: %s (code %d)", icikt_last_error(ctx), rc);
  const char *nm_t[] = {"rho", "pvalue", "n_values", "reason", "kernel_ms", ""};
  const char *nm[] = {"rho", "pvalue", "n_values", "reason", ""};
  SEXP res = PROTECT(Rf_mkNamed(VECSXP, with_timing ? nm_t : nm));
  for (int f = 0; f < 3; ++f) {   /* NA_real_ for the NA pairs: R's own NA payload */
    SEXP v = PROTECT(Rf_allocVector(REALSXP, P));
    for (int64_t p = 0; p < P; ++p) {
      const double d = out3[3 * p + f];
      REAL(v)[p] = (d != d) ? na_real() : d;
    }
    SET_VECTOR_ELT(res, f, v);
    UNPROTECT(1);
  }
  SEXP r = PROTECT(Rf_allocVector(INTSXP, P));
  for (int64_t p = 0; p < P; ++p) INTEGER(r)[p] = reasons[p];
  SET_VECTOR_ELT(res, 3, r);
  UNPROTECT(1);
  if (with_timing) {
    SEXP t = PROTECT(Rf_allocVector(REALSXP, ICIKT_K_COUNT));
    for (int k = 0; k < ICIKT_K_COUNT; ++k) {
      double ms = 0.0;
      int64_t launches = 0;
      icikt_kernel_ms(ctx, k, &ms, &launches);
      REAL(t)[k] = ms;
    }
    SET_VECTOR_ELT(res, 4, t);
    UNPROTECT(1);
  }
  UNPROTECT(1);
  return res;
}

static const R_CallMethodDef CallEntries[] = {
    {"icikt_R_cor", (DL_FUNC)&icikt_R_cor, 9},
    {NULL, NULL, 0}};

void R_init_icikt_rglue_cor(DllInfo *dll) {
  R_registerRoutines(dll, NULL, CallEntries, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}

void R_unload_icikt_rglue_cor(DllInfo *dll) {
  (void)dll;
  if (g_cor_ctx) { icikt_ctx_destroy(g_cor_ctx); g_cor_ctx = NULL; }
}
