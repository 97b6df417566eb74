/*
 * Rcpp.h -- a stand-in for the part of Rcpp that the reference's src/kendallc.cpp uses.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/ref_wrap.cpp includes the reference's file through an include path and this
 * header answers its `#include <Rcpp.h>`).  Written from Rcpp's documented behaviour, not from its sources: vectors
 * have VALUE semantics (the reference never relies on two names sharing storage: it clones before it writes), the
 * "sugar" functions are eager, and of R itself only pnorm is needed.
 *
 * What it CLAIMS Rcpp does, and tests/test_rcpp_standin_host.py states against numpy (DESIGN.md section 6 lists them as
 * readings -- Rcpp is not on the machine):
 *   - IntegerVector element operations and sum(IntegerVector) work in int: NA_INTEGER (INT_MIN) propagates, anything
 *     else wraps modulo 2^32 (done through unsigned here, so the stand-in has no undefined behaviour; gcc compiles
 *     Rcpp's signed arithmetic to the same instructions, and the -fwrapv build of the reference pins that);
 *   - `int / int` on the result of sum() is C's: it truncates toward zero;
 *   - sum(NumericVector) accumulates in double, sum(LogicalVector) counts TRUE;
 *   - table() is ordered by key, -0.0 and +0.0 are one key; duplicated() marks every occurrence but the first;
 *   - is_na() is true for NaN and for NA_real_; na_omit() drops both;
 *   - pnorm is R's: the lower or upper tail of the standard normal with the cut-off at |z| = 37.5193 beyond which the
 *     vanishing tail is exactly 0.  Here it is erfcl in long double, which is rounded better than R's Cody (1969)
 *     rational approximations; the difference is measured, not asserted away (profiles/epilogue_tails.md).
 */
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace Rcpp {

namespace standin {
inline double na_real() {                     // R's NA_real_: a NaN whose low word is 1954
  const uint64_t bits = 0x7FF00000000007A2ull;
  double d;
  std::memcpy(&d, &bits, sizeof d);
  return d;
}
inline std::string& captured() { static std::string s; return s; }        // what Rcout / Rprintf wrote
inline int& warnings() { static int n = 0; return n; }                    // how often warning() was called
inline std::string& last_warning() { static std::string s; return s; }
/* +0.0 for either zero, the value itself otherwise: the key under which table / unique / duplicated file a double */
inline double zero_key(double v) { return v == 0.0 ? 0.0 : v; }
}  // namespace standin

#define NA_REAL (::Rcpp::standin::na_real())
#define NA_INTEGER INT_MIN

struct IntegerTag {};
struct LogicalTag {};
struct NumericTag {};
template <typename T, typename Tag> class Vector;
typedef Vector<int, IntegerTag> IntegerVector;
typedef Vector<int, LogicalTag> LogicalVector;
typedef Vector<double, NumericTag> NumericVector;

class CharacterVector {
 public:
  CharacterVector() {}
  CharacterVector(std::initializer_list<const char*> l) : v_(l.begin(), l.end()) {}
  long size() const { return (long)v_.size(); }
  const std::string& operator[](long i) const { return v_[(size_t)i]; }

 private:
  std::vector<std::string> v_;
};

class String {
 public:
  String(const char* c) : s_(c) {}
  String(const std::string& c) : s_(c) {}
  bool operator==(const char* c) const { return s_ == c; }
  bool operator!=(const char* c) const { return s_ != c; }

 private:
  std::string s_;
};

/* v[integer vector] and v[logical vector]: reads as the selected elements, `= scalar` writes them in place */
template <typename T, typename Tag> class Subset {
 public:
  Subset(Vector<T, Tag>& src, std::vector<long> at) : src_(src), at_(std::move(at)) {}
  operator Vector<T, Tag>() const {
    Vector<T, Tag> r((long)at_.size());
    for (size_t k = 0; k < at_.size(); ++k) r[(long)k] = src_[at_[k]];
    return r;
  }
  Subset& operator=(T value) {
    for (long k : at_) src_[k] = value;
    return *this;
  }

 private:
  Vector<T, Tag>& src_;
  std::vector<long> at_;
};

template <typename T, typename Tag> class Vector {
 public:
  typedef typename std::vector<T>::iterator iterator;
  typedef typename std::vector<T>::const_iterator const_iterator;

  Vector() {}
  /* Vector(n): n zeros.  n may be any arithmetic type (the reference sizes one by a double) */
  template <typename U, typename = typename std::enable_if<std::is_arithmetic<U>::value>::type>
  Vector(U n) : d_((size_t)n, T(0)) {}
  template <typename U, typename = typename std::enable_if<std::is_arithmetic<U>::value>::type>
  Vector(U n, T fill) : d_((size_t)n, fill) {}
  Vector(std::initializer_list<T> l) : d_(l) {}
  /* the one cross-type conversion: an IntegerVector where a NumericVector is declared */
  template <typename Tag2, typename = typename std::enable_if<std::is_same<Tag, NumericTag>::value &&
                                                              std::is_same<Tag2, IntegerTag>::value>::type>
  Vector(const Vector<int, Tag2>& o) : d_(o.begin(), o.end()) {
    for (long k = 0; k < o.size(); ++k)
      if (o[k] == NA_INTEGER) d_[(size_t)k] = NA_REAL;
  }
  static Vector create(T a) { return Vector({a}); }
  static Vector create(T a, T b) { return Vector({a, b}); }
  static Vector create(T a, T b, T c) { return Vector({a, b, c}); }

  long size() const { return (long)d_.size(); }
  long length() const { return (long)d_.size(); }
  iterator begin() { return d_.begin(); }
  iterator end() { return d_.end(); }
  const_iterator begin() const { return d_.begin(); }
  const_iterator end() const { return d_.end(); }
  T& operator[](long i) { return d_[(size_t)i]; }
  const T& operator[](long i) const { return d_[(size_t)i]; }
  T& operator()(long i) { return d_[(size_t)i]; }
  const T& operator()(long i) const { return d_[(size_t)i]; }
  Subset<T, Tag> operator[](const IntegerVector& at) {
    return Subset<T, Tag>(*this, std::vector<long>(at.begin(), at.end()));
  }
  Subset<T, Tag> operator[](const LogicalVector& keep) {
    std::vector<long> at;
    for (long k = 0; k < keep.size(); ++k)
      if (keep[k] == 1) at.push_back(k);
    return Subset<T, Tag>(*this, std::move(at));
  }
  void push_back(T v) { d_.push_back(v); }
  CharacterVector& names() { return names_; }

 private:
  std::vector<T> d_;
  CharacterVector names_;
};

/* ---- element arithmetic ------------------------------------------------------------------------------------------- */
namespace standin {
struct Add {
  static int i(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
  static double d(double a, double b) { return a + b; }
};
struct Sub {
  static int i(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
  static double d(double a, double b) { return a - b; }
};
struct Mul {
  static int i(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
  static double d(double a, double b) { return a * b; }
};
struct Div {
  static int i(int a, int b) { return b == 0 || (a == INT_MIN && b == -1) ? NA_INTEGER : a / b; }   // C's: truncates
  static double d(double a, double b) { return a / b; }
};
template <typename Op> int int_op(int a, int b) { return a == NA_INTEGER || b == NA_INTEGER ? NA_INTEGER : Op::i(a, b); }
template <typename Op> IntegerVector map(const IntegerVector& a, const IntegerVector& b) {
  if (a.size() != b.size()) throw std::range_error("sugar: vectors of different length");
  IntegerVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = int_op<Op>(a[k], b[k]);
  return r;
}
template <typename Op> IntegerVector map(const IntegerVector& a, int b) {
  IntegerVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = int_op<Op>(a[k], b);
  return r;
}
template <typename Op> IntegerVector map(int a, const IntegerVector& b) {
  IntegerVector r(b.size());
  for (long k = 0; k < b.size(); ++k) r[k] = int_op<Op>(a, b[k]);
  return r;
}
template <typename Op> NumericVector map(const NumericVector& a, const NumericVector& b) {
  if (a.size() != b.size()) throw std::range_error("sugar: vectors of different length");
  NumericVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = Op::d(a[k], b[k]);
  return r;
}
template <typename Op> NumericVector map(const NumericVector& a, double b) {
  NumericVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = Op::d(a[k], b);
  return r;
}
template <typename Op> NumericVector map(double a, const NumericVector& b) {
  NumericVector r(b.size());
  for (long k = 0; k < b.size(); ++k) r[k] = Op::d(a, b[k]);
  return r;
}
}  // namespace standin

#define RCPP_STANDIN_OPERATOR(sym, Op)                                                                              \
  inline IntegerVector operator sym(const IntegerVector& a, const IntegerVector& b) { return standin::map<standin::Op>(a, b); } \
  inline IntegerVector operator sym(const IntegerVector& a, int b) { return standin::map<standin::Op>(a, b); }      \
  inline IntegerVector operator sym(int a, const IntegerVector& b) { return standin::map<standin::Op>(a, b); }      \
  inline NumericVector operator sym(const NumericVector& a, const NumericVector& b) { return standin::map<standin::Op>(a, b); } \
  inline NumericVector operator sym(const NumericVector& a, double b) { return standin::map<standin::Op>(a, b); }   \
  inline NumericVector operator sym(double a, const NumericVector& b) { return standin::map<standin::Op>(a, b); }
RCPP_STANDIN_OPERATOR(+, Add)
RCPP_STANDIN_OPERATOR(-, Sub)
RCPP_STANDIN_OPERATOR(*, Mul)
RCPP_STANDIN_OPERATOR(/, Div)
#undef RCPP_STANDIN_OPERATOR

inline LogicalVector operator&(const LogicalVector& a, const LogicalVector& b) {
  LogicalVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = a[k] && b[k];
  return r;
}
inline LogicalVector operator|(const LogicalVector& a, const LogicalVector& b) {
  LogicalVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = a[k] || b[k];
  return r;
}
inline LogicalVector operator!(const LogicalVector& a) {
  LogicalVector r(a.size());
  for (long k = 0; k < a.size(); ++k) r[k] = !a[k];
  return r;
}

/* ---- sugar -------------------------------------------------------------------------------------------------------- */
inline LogicalVector is_na(const NumericVector& x) {
  LogicalVector r(x.size());
  for (long k = 0; k < x.size(); ++k) r[k] = std::isnan(x[k]) ? 1 : 0;
  return r;
}
inline NumericVector na_omit(const NumericVector& x) {
  NumericVector r;
  for (double v : x)
    if (!std::isnan(v)) r.push_back(v);
  return r;
}
inline int sum(const LogicalVector& x) {
  int s = 0;
  for (int v : x) s += v;
  return s;
}
inline int sum(const IntegerVector& x) {
  unsigned s = 0;
  for (int v : x) {
    if (v == NA_INTEGER) return NA_INTEGER;
    s += (unsigned)v;
  }
  return (int)s;
}
inline double sum(const NumericVector& x) {
  double s = 0;
  for (double v : x) s += v;
  return s;
}
template <typename T, typename Tag> Vector<T, Tag> clone(const Vector<T, Tag>& x) { return x; }
inline double min(const NumericVector& x) {
  if (x.size() == 0) return INFINITY;
  double m = x[0];
  for (double v : x) {
    if (std::isnan(v)) return v;
    if (v < m) m = v;
  }
  return m;
}
inline int max(const IntegerVector& x) {
  if (x.size() == 0) throw std::range_error("max of an empty integer vector");
  int m = x[0];
  for (int v : x)
    if (v > m) m = v;
  return m;
}
template <typename T, typename Tag> IntegerVector seq_along(const Vector<T, Tag>& x) {
  IntegerVector r(x.size());
  for (long k = 0; k < x.size(); ++k) r[k] = (int)k + 1;
  return r;
}
inline IntegerVector seq(int from, int to) {
  if (to < from) throw std::range_error("upper value must be greater than lower value");
  IntegerVector r(to - from + 1);
  for (int k = from; k <= to; ++k) r[k - from] = k;
  return r;
}
inline NumericVector unique(const NumericVector& x) {       // first occurrences, in order; every NaN is one value
  NumericVector r;
  std::set<double> seen;
  bool seen_nan = false;
  for (double v : x) {
    if (std::isnan(v)) {
      if (!seen_nan) r.push_back(v);
      seen_nan = true;
    } else if (seen.insert(standin::zero_key(v)).second) {
      r.push_back(v);
    }
  }
  return r;
}
inline IntegerVector cumsum(const IntegerVector& x) {
  IntegerVector r(x.size());
  int s = 0;
  for (long k = 0; k < x.size(); ++k) {
    s = standin::int_op<standin::Add>(s, x[k]);
    r[k] = s;
  }
  return r;
}
inline IntegerVector diff(const IntegerVector& x) {
  IntegerVector r(x.size() > 0 ? x.size() - 1 : 0);
  for (long k = 0; k + 1 < x.size(); ++k) r[k] = standin::int_op<standin::Sub>(x[k + 1], x[k]);
  return r;
}
inline LogicalVector duplicated(const IntegerVector& x) {
  LogicalVector r(x.size());
  std::set<int> seen;
  for (long k = 0; k < x.size(); ++k) r[k] = seen.insert(x[k]).second ? 0 : 1;
  return r;
}
inline LogicalVector duplicated(const NumericVector& x) {   // (NaN-free input: the reference fills before it calls)
  LogicalVector r(x.size());
  std::set<double> seen;
  for (long k = 0; k < x.size(); ++k) r[k] = seen.insert(standin::zero_key(x[k])).second ? 0 : 1;
  return r;
}
inline IntegerVector table(const IntegerVector& x) {        // counts, in ascending order of the key
  std::map<int, int> m;
  for (int v : x) ++m[v];
  IntegerVector r;
  for (const auto& kv : m) r.push_back(kv.second);
  return r;
}
inline IntegerVector table(const NumericVector& x) {
  std::map<double, int> m;
  for (double v : x) ++m[standin::zero_key(v)];
  IntegerVector r;
  for (const auto& kv : m) r.push_back(kv.second);
  return r;
}

/* R's pnorm(q, mean, sd, lower_tail, log_p), element-wise */
inline NumericVector pnorm(const NumericVector& q, double mean = 0.0, double sd = 1.0, bool lower = true,
                           bool log_p = false) {
  NumericVector r(q.size());
  for (long k = 0; k < q.size(); ++k) {
    const long double z = ((long double)q[k] - mean) / sd;
    if (std::isnan((double)z)) {
      r[k] = (double)z;
      continue;
    }
    const long double a = fabsl(z);
    const long double small = a >= 37.5193L ? 0.0L : 0.5L * erfcl(a / sqrtl(2.0L));   // the tail that vanishes
    const long double p = (z < 0) == lower ? small : (z == 0 ? 0.5L : 1.0L - small);
    r[k] = (double)(log_p ? logl(p) : p);
  }
  return r;
}

/* ---- R's side: errors, warnings, output ------------------------------------------------------------------------------ */
inline void stop(const char* msg) { throw std::runtime_error(msg); }
inline void warning(const char* msg) {
  ++standin::warnings();
  standin::last_warning() = msg;
}
struct Ostream {
  Ostream& operator<<(const std::string& s) {
    standin::captured() += s;
    return *this;
  }
  Ostream& operator<<(const char* s) {
    standin::captured() += s;
    return *this;
  }
};
static Ostream Rcout __attribute__((unused));

}  // namespace Rcpp

__attribute__((format(printf, 1, 2))) inline void Rprintf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  Rcpp::standin::captured() += buf;
}
