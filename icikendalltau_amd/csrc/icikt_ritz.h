// icikt_ritz.h -- the host arithmetic of icikt_pcoa_* (DESIGN.md section 27): the symmetric eigen-solver of the
// projected L x L problem, and the correctly rounded conversion of a ratio of integers to a double.  Plain C++ without a
// device header, like icikt_blocks.h: tests/test_ritz_host.py compiles it alone (tests/ritz_print.cpp) and holds it
// against numpy.linalg.eigh and Python's int / int.
#ifndef ICIKT_RITZ_H
#define ICIKT_RITZ_H

#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace icikt {
namespace ritz {

typedef unsigned __int128 u128;

inline int bit_length(u128 v) {
  const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
  if (hi) return 128 - __builtin_clzll(hi);
  return lo ? 64 - __builtin_clzll(lo) : 0;
}

// The double nearest to num / den, ties to even (Python's int / int).  den > 0; the odd part of den is below 2^64 and
// num below 2^100 (this entry: num < 2^84, den = S 2^50 or S^2 2^50).  The quotient is taken to at least 55 bits with
// the remainder as a sticky bit, rounded once to 53 bits, and scaled by a power of two, which is exact: every result
// here is far from the subnormal range.
inline double ratio_to_double(u128 num, u128 den) {
  if (num == 0) return 0.0;
  int e = 0;
  while ((den & 1) == 0) { den >>= 1; --e; }           // a power of two in the divisor only moves the exponent
  const int s = 56 + bit_length(den) - bit_length(num);  // num 2^s / den has 56 or 57 bits
  if (s > 0) { num <<= s; e -= s; }
  u128 q = num / den;
  const bool sticky = (num % den) != 0;
  const int drop = bit_length(q) - 53;                 // >= 2 with s > 0; a long quotient drops more
  if (drop > 0) {
    const u128 half = (u128)1 << (drop - 1);
    const u128 low = q & ((half << 1) - 1);
    q >>= drop;
    if (low > half || (low == half && (sticky || (q & 1)))) q += 1;
    e += drop;
  }
  return std::ldexp((double)(unsigned long long)q, e);   // q <= 2^53: exact
}

// Eigenvalues (ascending, w [L]) and orthonormal eigenvectors (the columns of Z: Z[i * L + j] is component i of vector
// j) of the symmetric H [L][L] (row-major; the lower triangle is read).  Householder tridiagonalisation and implicit QL
// (EISPACK's tred2 / tql2 in the form of the public-domain JAMA library).  Returns false if an eigenvalue has not
// converged within 60 iterations.
inline bool sym_eig(const double* H, int L, double* w, double* Z) {
  const int n = L;
  if (n <= 0) return true;
  std::vector<double> e((size_t)n, 0.0);
  double* V = Z;
  double* d = w;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[(size_t)i * n + j] = j <= i ? H[(size_t)i * n + j] : H[(size_t)j * n + i];
#define ICIKT_V(i, j) V[(size_t)(i) * n + (j)]
  // --- tred2 ---
  for (int j = 0; j < n; ++j) d[j] = ICIKT_V(n - 1, j);
  for (int i = n - 1; i > 0; --i) {
    double scale = 0.0, h = 0.0;
    for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
    if (scale == 0.0) {
      e[i] = d[i - 1];
      for (int j = 0; j < i; ++j) {
        d[j] = ICIKT_V(i - 1, j);
        ICIKT_V(i, j) = 0.0;
        ICIKT_V(j, i) = 0.0;
      }
    } else {
      for (int k = 0; k < i; ++k) {
        d[k] /= scale;
        h += d[k] * d[k];
      }
      double f = d[i - 1];
      double g = std::sqrt(h);
      if (f > 0) g = -g;
      e[i] = scale * g;
      h -= f * g;
      d[i - 1] = f - g;
      for (int j = 0; j < i; ++j) e[j] = 0.0;
      for (int j = 0; j < i; ++j) {
        f = d[j];
        ICIKT_V(j, i) = f;
        g = e[j] + ICIKT_V(j, j) * f;
        for (int k = j + 1; k <= i - 1; ++k) {
          g += ICIKT_V(k, j) * d[k];
          e[k] += ICIKT_V(k, j) * f;
        }
        e[j] = g;
      }
      f = 0.0;
      for (int j = 0; j < i; ++j) {
        e[j] /= h;
        f += e[j] * d[j];
      }
      const double hh = f / (h + h);
      for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (int j = 0; j < i; ++j) {
        f = d[j];
        g = e[j];
        for (int k = j; k <= i - 1; ++k) ICIKT_V(k, j) -= (f * e[k] + g * d[k]);
        d[j] = ICIKT_V(i - 1, j);
        ICIKT_V(i, j) = 0.0;
      }
    }
    d[i] = h;
  }
  for (int i = 0; i < n - 1; ++i) {
    ICIKT_V(n - 1, i) = ICIKT_V(i, i);
    ICIKT_V(i, i) = 1.0;
    const double h = d[i + 1];
    if (h != 0.0) {
      for (int k = 0; k <= i; ++k) d[k] = ICIKT_V(k, i + 1) / h;
      for (int j = 0; j <= i; ++j) {
        double g = 0.0;
        for (int k = 0; k <= i; ++k) g += ICIKT_V(k, i + 1) * ICIKT_V(k, j);
        for (int k = 0; k <= i; ++k) ICIKT_V(k, j) -= g * d[k];
      }
    }
    for (int k = 0; k <= i; ++k) ICIKT_V(k, i + 1) = 0.0;
  }
  for (int j = 0; j < n; ++j) {
    d[j] = ICIKT_V(n - 1, j);
    ICIKT_V(n - 1, j) = 0.0;
  }
  ICIKT_V(n - 1, n - 1) = 1.0;
  e[0] = 0.0;
  // --- tql2 ---
  for (int i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  double f = 0.0, tst1 = 0.0;
  const double eps = std::ldexp(1.0, -52);
  for (int l = 0; l < n; ++l) {
    tst1 = std::fmax(tst1, std::fabs(d[l]) + std::fabs(e[l]));
    int m = l;
    while (m < n) {
      if (std::fabs(e[m]) <= eps * tst1) break;
      ++m;
    }
    if (m >= n) m = n - 1;
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 60) return false;
        double g = d[l];
        double p = (d[l + 1] - g) / (2.0 * e[l]);
        double r = std::hypot(p, 1.0);
        if (p < 0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (int i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c;
        const double el1 = e[l + 1];
        double s = 0.0, s2 = 0.0;
        for (int i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = std::hypot(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (int k = 0; k < n; ++k) {
            h = ICIKT_V(k, i + 1);
            ICIKT_V(k, i + 1) = s * ICIKT_V(k, i) + c * h;
            ICIKT_V(k, i) = c * ICIKT_V(k, i) - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (std::fabs(e[l]) > eps * tst1);
    }
    d[l] = d[l] + f;
    e[l] = 0.0;
  }
  // ascending, by selection: equal values keep their order
  for (int i = 0; i < n - 1; ++i) {
    int k = i;
    double p = d[i];
    for (int j = i + 1; j < n; ++j)
      if (d[j] < p) { k = j; p = d[j]; }
    if (k != i) {
      d[k] = d[i];
      d[i] = p;
      for (int j = 0; j < n; ++j) std::swap(ICIKT_V(j, i), ICIKT_V(j, k));
    }
  }
#undef ICIKT_V
  return true;
}

}  // namespace ritz
}  // namespace icikt
#endif
