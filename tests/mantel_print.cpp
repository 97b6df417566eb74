// mantel_print.cpp -- prints what csrc/icikt_mantel.h makes of the words it reads from standard input, as JSON, for
// tests/test_mantel_host.py.  Host code only: no device header, no library.  Input lines:
//   x <bits>                      a raw value (the bits of a double, as an unsigned decimal word)
//   y <bits>                      a value of `other`
//   c <lo_a> <hi_a> <lo_b> <hi_b> two limb sums to compare
// Output:
//   "xv"       mantel::quantise_x(raw), null for a NaN
//   "xv_key"   mantel::quantise_x(mantel::key_value(host::cor_key(raw))): the way the device takes it, through the kept key
//   "lo", "hi", "span"   the bits of the smallest and largest y and of hi - lo; "e": mantel::span_exponent(span)
//   "yv"       mantel::quantise_y(y, lo, e)
//   "t"        the limb sums [lo, hi] of xv[k] yv[k] over the first min(#x, #y) values (NaN: 0), as the kernel adds them
//   "mx", "my" [s_lo, s_hi, q_lo, q_hi]: the limb sums of v and v^2
//   "cmp"      mantel::compare_sums per c line
// and the header's constants.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icikt_keys.h"
#include "icikt_mantel.h"

using namespace icikt;

static void print_list(const char* name, const std::vector<long long>& v, const char* tail) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) {
    if (v[i] < 0) std::printf("%snull", i ? ", " : "");
    else std::printf("%s%lld", i ? ", " : "", v[i]);
  }
  std::printf("]%s", tail);
}

static void moments(const std::vector<long long>& v, unsigned long long out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0ull;
  for (long long s : v) {
    const unsigned long long u = s < 0 ? 0ull : (unsigned long long)s, q = u * u;
    out[0] += mantel::limb_lo(u);
    out[1] += mantel::limb_hi(u);
    out[2] += mantel::limb_lo(q);
    out[3] += mantel::limb_hi(q);
  }
}

int main() {
  std::vector<double> xs, ys;
  std::vector<int> cmp;
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    if (line[0] == 'x' || line[0] == 'y') {
      char* end = nullptr;
      const unsigned long long w = std::strtoull(line + 1, &end, 10);
      if (end == line + 1) return 2;
      (line[0] == 'x' ? xs : ys).push_back(host::from_bits(w));
    } else if (line[0] == 'c') {
      unsigned long long a[4];
      if (std::sscanf(line + 1, "%llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3]) != 4) return 2;
      cmp.push_back(mantel::compare_sums(a[0], a[1], a[2], a[3]));
    } else {
      return 2;
    }
  }
  std::vector<long long> xv, xk, yv;
  for (double raw : xs) {
    xv.push_back(raw != raw ? -1 : (long long)mantel::quantise_x(raw));
    const unsigned long long k = host::cor_key(raw);
    xk.push_back(k == host::NA_KEY ? -1 : (long long)mantel::quantise_x(mantel::key_value(k)));
  }
  double lo = 0.0, hi = 0.0;
  for (size_t p = 0; p < ys.size(); ++p) {
    if (p == 0 || ys[p] < lo) lo = ys[p];
    if (p == 0 || ys[p] > hi) hi = ys[p];
  }
  const double span = hi - lo;
  const int e = mantel::span_exponent(span);
  for (double y : ys) yv.push_back((long long)mantel::quantise_y(y, lo, e));
  unsigned long long t_lo = 0ull, t_hi = 0ull;
  for (size_t k = 0; k < xv.size() && k < yv.size(); ++k) {
    const unsigned long long prod = (unsigned long long)(xk[k] < 0 ? 0 : xk[k]) * (unsigned long long)yv[k];
    t_lo += mantel::limb_lo(prod);
    t_hi += mantel::limb_hi(prod);
  }
  unsigned long long mx[4], my[4];
  moments(xk, mx);
  moments(yv, my);
  std::printf("{\"x_frac_bits\": %d, \"y_bits\": %d, \"v_max\": %llu, \"methods\": [%d, %d], ", mantel::X_FRAC_BITS,
              mantel::Y_BITS, mantel::V_MAX, mantel::METHOD_PEARSON, mantel::METHOD_SPEARMAN);
  print_list("xv", xv, ", ");
  print_list("xv_key", xk, ", ");
  std::printf("\"lo\": %llu, \"hi\": %llu, \"span\": %llu, \"e\": %d, ", host::bits_of(lo), host::bits_of(hi),
              host::bits_of(span), e);
  print_list("yv", yv, ", ");
  std::printf("\"t\": [%llu, %llu], \"mx\": [%llu, %llu, %llu, %llu], \"my\": [%llu, %llu, %llu, %llu], \"cmp\": [", t_lo, t_hi,
              mx[0], mx[1], mx[2], mx[3], my[0], my[1], my[2], my[3]);
  for (size_t i = 0; i < cmp.size(); ++i) std::printf("%s%d", i ? ", " : "", cmp[i]);
  std::printf("], \"limbs\": [%llu, %llu]}\n", mantel::limb_lo(0xFEDCBA9876543210ull), mantel::limb_hi(0xFEDCBA9876543210ull));
  return 0;
}
