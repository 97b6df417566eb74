// ritz_print.cpp -- prints what csrc/icikt_ritz.h makes of the lines it reads from standard input, one answer per line,
// for tests/test_ritz_host.py.  Host code only: no device header, no library.
//   r <num_hi> <num_lo> <den_hi> <den_lo>   (unsigned decimal 64-bit halves)  -> the bits of ratio_to_double(num, den)
//   e <L> then L * L words (the bits of H, row-major), one per line           -> "ok" or "fail", then the bits of the L
//                                                                                eigenvalues and of Z [L][L], one line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icikt_ritz.h"

using namespace icikt;

static unsigned long long bits_of(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

static double from_bits(unsigned long long b) {
  double v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    if (line[0] == 'r') {
      unsigned long long nh, nl, dh, dl;
      if (std::sscanf(line + 1, "%llu %llu %llu %llu", &nh, &nl, &dh, &dl) != 4) return 2;
      const ritz::u128 num = ((ritz::u128)nh << 64) | nl, den = ((ritz::u128)dh << 64) | dl;
      std::printf("%llu\n", bits_of(ritz::ratio_to_double(num, den)));
    } else if (line[0] == 'e') {
      const int L = std::atoi(line + 1);
      if (L < 1 || L > 4096) return 2;
      std::vector<double> H((size_t)L * L), w((size_t)L), Z((size_t)L * L);
      for (size_t i = 0; i < H.size(); ++i) {
        if (!std::fgets(line, sizeof line, stdin)) return 2;
        H[i] = from_bits(std::strtoull(line, nullptr, 10));
      }
      const bool ok = ritz::sym_eig(H.data(), L, w.data(), Z.data());
      std::printf("%s", ok ? "ok" : "fail");
      for (double v : w) std::printf(" %llu", bits_of(v));
      for (double v : Z) std::printf(" %llu", bits_of(v));
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
