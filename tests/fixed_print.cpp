// fixed_print.cpp -- prints what csrc/icikt_fixed.h makes of the doubles whose bits it reads from standard input (one
// unsigned decimal word per line), as JSON, for tests/test_fixed_host.py.  Host code only: no device header, no library.
//   "q"       fixed::quantise(raw)
//   "q_key"   fixed::quantise_key(host::cor_key(raw)): the way the device takes it, through the kept key
//   "back"    the bits of fixed::key_value(host::cor_key(raw))
// and the header's constants.  A NaN (its key is NA_KEY) gives q null, q_key 0 and back null.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icikt_fixed.h"
#include "icikt_keys.h"

using namespace icikt;

int main() {
  std::vector<unsigned long long> words;
  char line[64];
  while (std::fgets(line, sizeof line, stdin)) {
    char* end = nullptr;
    words.push_back(std::strtoull(line, &end, 10));
    if (end == line) return 2;
  }
  std::printf("{\"frac_bits\": %d, \"q_max\": %llu, \"na_key\": %llu, \"q\": [", fixed::FRAC_BITS, fixed::Q_MAX, fixed::NA_KEY);
  for (size_t i = 0; i < words.size(); ++i) {
    const double raw = host::from_bits(words[i]);
    if (raw != raw) std::printf("%snull", i ? ", " : "");
    else std::printf("%s%llu", i ? ", " : "", fixed::quantise(raw));
  }
  std::printf("], \"q_key\": [");
  for (size_t i = 0; i < words.size(); ++i)
    std::printf("%s%llu", i ? ", " : "", fixed::quantise_key(host::cor_key(host::from_bits(words[i]))));
  std::printf("], \"back\": [");
  for (size_t i = 0; i < words.size(); ++i) {
    const unsigned long long k = host::cor_key(host::from_bits(words[i]));
    if (k == host::NA_KEY) std::printf("%snull", i ? ", " : "");
    else std::printf("%s%llu", i ? ", " : "", host::bits_of(fixed::key_value(k)));
  }
  std::printf("], \"limbs\": [%llu, %llu]}\n", fixed::limb_lo(0x123456789ABCDEFull), fixed::limb_hi(0x123456789ABCDEFull));
  return 0;
}
