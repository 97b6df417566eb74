/*
 * ref_wrap.cpp -- C entry points around the reference's own src/kendallc.cpp (TEST INFRASTRUCTURE ONLY).
 *
 * The reference's file is included through the include path (`make ref` passes -I$(ICIKT_REFERENCE_DIR)/src), never
 * copied; its own include of Rcpp.h finds oracle/rcpp_standin/Rcpp.h.  Nothing built from this file is committed
 * (oracle/_ref/ is ignored) and the product package never loads it.  Not thread safe: the stand-in keeps the captured
 * report and the warning count in statics.
 */
#include "Rcpp.h"

#include "kendallc.cpp"

namespace {
void reset() {
  Rcpp::standin::captured().clear();
  Rcpp::standin::warnings() = 0;
  Rcpp::standin::last_warning().clear();
}
void copy_text(const std::string& s, char* buf, long cap) {
  if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", s.c_str());
}
}  // namespace

extern "C" {

/* ici_kt(x, y, perspective, alternative, continuity, output).  out4 = tau, pvalue, tau_max, completeness; report_buf
   receives what the call wrote to Rcout (want_report != 0) or the message of the exception (return value 1). */
int ref_ici_kt(const double* x, const double* y, long n, const char* perspective, const char* alternative,
               int continuity, int want_report, double* out4, char* report_buf, long cap, int* n_warnings) {
  reset();
  NumericVector X(n), Y(n);
  for (long k = 0; k < n; ++k) {
    X[k] = x[k];
    Y[k] = y[k];
  }
  try {
    NumericVector r = ici_kt(X, Y, String(perspective), String(alternative), continuity != 0,
                             String(want_report ? "report" : "simple"));
    for (int k = 0; k < 4; ++k) out4[k] = r[k];
  } catch (const std::exception& e) {
    copy_text(e.what(), report_buf, cap);
    return 1;
  }
  copy_text(Rcpp::standin::captured(), report_buf, cap);
  if (n_warnings) *n_warnings = Rcpp::standin::warnings();
  return 0;
}

/* the text of the last warning of the last ref_ici_kt call ("" when it raised none) */
void ref_last_warning(char* buf, long cap) { copy_text(Rcpp::standin::last_warning(), buf, cap); }

/* The reference's own chain on one already filled column (no NaN): sortedIndex -> subset -> compare_self -> cumsum ->
   count_rank_tie.  out3 = the three sums it returns (ici_kt reads them as xtie, x0, x1). */
int ref_count_rank_tie(const double* col, long n, double* out3) {
  reset();
  if (n < 1) return 2;
  try {
    NumericVector v(n);
    for (long k = 0; k < n; ++k) v[k] = col[k];
    IntegerVector perm = sortedIndex(v);
    v = v[perm];
    IntegerVector ranks = cumsum(compare_self(v));
    NumericVector c = count_rank_tie(ranks);
    for (int k = 0; k < 3; ++k) out3[k] = c[k];
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}

/* kendall_discordant on dense ranks (x4 ascending, y4 >= 1), as ici_kt calls it */
int ref_kendall_discordant(const int* x4, const int* y4, long n) {
  IntegerVector X(n), Y(n);
  for (long k = 0; k < n; ++k) {
    X[k] = x4[k];
    Y[k] = y4[k];
  }
  return kendall_discordant(X, Y);
}

}  // extern "C"
