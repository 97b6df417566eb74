// Prints what oracle/rcpp_standin/Rcpp.h makes of the numbers on its command line, as JSON, for
// tests/test_rcpp_standin_host.py.  usage: rcpp_standin_print MODE list [-- list ...]; integers are decimal, doubles are
// the decimal value of their 64-bit pattern (in and out), so that NaN payloads and -0.0 survive.
#include "Rcpp.h"

#include <cinttypes>
#include <cstdlib>
#include <string>
#include <vector>

using Rcpp::IntegerVector;
using Rcpp::LogicalVector;
using Rcpp::NumericVector;
using Rcpp::CharacterVector;
using Rcpp::String;
namespace standin = Rcpp::standin;

static double from_word(uint64_t w) {
  double d;
  std::memcpy(&d, &w, sizeof d);
  return d;
}
static uint64_t to_word(double d) {
  uint64_t w;
  std::memcpy(&w, &d, sizeof w);
  return w;
}
static IntegerVector ints(const std::vector<std::string>& a) {
  IntegerVector v;
  for (const auto& s : a) v.push_back((int)strtol(s.c_str(), nullptr, 10));
  return v;
}
static LogicalVector lgls(const std::vector<std::string>& a) {
  LogicalVector v;
  for (const auto& s : a) v.push_back((int)strtol(s.c_str(), nullptr, 10));
  return v;
}
static NumericVector dbls(const std::vector<std::string>& a) {
  NumericVector v;
  for (const auto& s : a) v.push_back(from_word(strtoull(s.c_str(), nullptr, 10)));
  return v;
}
static void put(const char* key, const IntegerVector& v, bool last = false) {
  printf("\"%s\": [", key);
  for (long k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
  printf("]%s", last ? "" : ", ");
}
static void put(const char* key, const LogicalVector& v, bool last = false) {
  printf("\"%s\": [", key);
  for (long k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
  printf("]%s", last ? "" : ", ");
}
static void put(const char* key, const NumericVector& v, bool last = false) {
  printf("\"%s\": [", key);
  for (long k = 0; k < v.size(); ++k) printf("%s%" PRIu64, k ? ", " : "", to_word(v[k]));
  printf("]%s", last ? "" : ", ");
}
static void put(const char* key, long v, bool last = false) { printf("\"%s\": %ld%s", key, v, last ? "" : ", "); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  std::vector<std::vector<std::string>> lists(1);
  for (int k = 2; k < argc; ++k) {
    if (std::string(argv[k]) == "--") lists.emplace_back();
    else lists.back().push_back(argv[k]);
  }
  lists.resize(3);
  printf("{");
  if (mode == "int") {                       // two integer vectors of one length, and the scalar lists[2][0]
    IntegerVector a = ints(lists[0]), b = ints(lists[1]);
    const int s = ints(lists[2])[0];
    put("add", a + b);
    put("sub", a - b);
    put("mul", a * b);
    put("add_s", a + s);
    put("sub_s", a - s);
    put("s_sub", s - a);
    put("mul_s", a * s);
    put("s_mul", s * a);
    put("div_s", a / s);
    put("cumsum", cumsum(a));
    put("diff", diff(a));
    put("table", table(a));
    put("duplicated", duplicated(a));
    put("which_dup", IntegerVector(a[duplicated(a)]));
    put("seq_along", seq_along(a));
    put("max", (long)max(a));
    const int total = sum(a);
    put("sum", (long)total);
    put("sum_half", (long)(total == NA_INTEGER ? NA_INTEGER : total / 2));
    // the expressions of the reference's count_rank_tie, on `a` as the group sizes
    put("tt1", (long)sum(a * (a - 1)));
    put("tt1_half", (long)(sum(a * (a - 1)) / 2));
    put("t0", (long)sum(a * (a - 1) * (a - 2)));
    put("t1", (long)sum(a * (a - 1) * (2 * a + 5)), true);
  } else if (mode == "real") {               // a double vector, an integer index into it, a logical mask over it
    NumericVector x = dbls(lists[0]);
    IntegerVector at = ints(lists[1]);
    LogicalVector keep = lgls(lists[2]);
    put("is_na", is_na(x));
    put("na_omit", na_omit(x));
    put("unique", unique(na_omit(x)));
    put("table", table(na_omit(x)));
    put("duplicated", duplicated(na_omit(x)));
    put("n_na", (long)sum(is_na(x)));
    put("by_int", NumericVector(x[at]));
    put("by_lgl", NumericVector(x[keep]));
    put("by_not", NumericVector(x[!keep]));
    put("and", keep & is_na(x));
    put("or", keep | is_na(x));
    NumericVector w = clone(x);
    w[keep] = 7.5;
    put("assigned", w);
    put("untouched", x);
    put("sum", NumericVector::create(sum(na_omit(x))));
    put("min", NumericVector::create(min(na_omit(x))));
    put("plus", na_omit(x) + 0.1);
    put("minus", na_omit(x) - 0.1);
    put("times", 2.0 * na_omit(x));
    put("over", na_omit(x) / 3.0);
    put("from_int", NumericVector(at), true);
  } else if (mode == "pnorm") {
    NumericVector z = dbls(lists[0]);
    put("lower", pnorm(z, 0.0, 1.0));
    put("lower_explicit", pnorm(z, 0.0, 1.0, true, false));
    put("upper", pnorm(z, 0.0, 1.0, false));
    put("upper_explicit", pnorm(z, 0.0, 1.0, false, false), true);
  } else if (mode == "misc") {
    put("na_real", NumericVector::create(NA_REAL));
    put("na_integer", (long)NA_INTEGER);
    put("seq", Rcpp::seq(0, 4));
    put("seq_one", Rcpp::seq(3, 3));
    long threw = 0;
    try {
      Rcpp::seq(0, -1);
    } catch (const std::range_error&) {
      threw = 1;
    }
    put("seq_empty_throws", threw);
    threw = 0;
    try {
      Rcpp::stop("stopped");
    } catch (const std::exception& e) {
      threw = std::string(e.what()) == "stopped";
    }
    put("stop_throws", threw);
    Rcpp::warning("first");
    Rcpp::warning("second");
    put("warnings", (long)standin::warnings());
    put("last_warning_is_second", (long)(standin::last_warning() == "second"));
    Rcpp::Rcout << std::string("a: 1\n");
    Rprintf("b: %f \n", 2.5);
    put("captured_ok", (long)(standin::captured() == "a: 1\nb: 2.500000 \n"));
    IntegerVector sized(3.0, 0);             // sized by a double, as the reference's Fenwick array is
    NumericVector zeros(4);
    put("sized", sized);
    put("zeros", zeros);
    NumericVector named(2);
    named.names() = CharacterVector({"tau", "pvalue"});
    put("names", named.names().size());
    NumericVector byd = {1.5, 2.5, 3.5};
    double i = 1;                            // the reference indexes with double variables
    put("double_index", NumericVector::create(byd[i], byd(2)));
    String s("local");
    put("string_eq", (long)((s == "local") && (s != "global") && !(s == "global")), true);
  } else {
    return 2;
  }
  printf("}\n");
  return 0;
}
