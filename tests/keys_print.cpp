// keys_print.cpp -- prints what csrc/icikt_keys.h makes of the 64-bit words on its command line, as JSON, for
// tests/test_keys_host.py.  Host code only: no device header, no library.
//   keys_print cor BITS...      the doubles with these bits: their cor_key, and the bits cor_key_value makes of that key
//                               (null for NA_KEY, which has no value); the header's two constants
//   keys_print taumax WORD...   the bits of max_taumax_of(word)
// Every word goes in and comes out as an unsigned decimal number.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icikt_keys.h"

using namespace icikt::host;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<unsigned long long> words;
  for (int a = 2; a < argc; ++a) {
    char* end = nullptr;
    words.push_back(std::strtoull(argv[a], &end, 10));
    if (!end || *end) return 2;
  }
  if (!std::strcmp(argv[1], "cor")) {
    std::printf("{\"na_key\": %llu, \"r_na_bits\": %llu, \"key\": [", NA_KEY, R_NA_BITS);
    for (size_t i = 0; i < words.size(); ++i) std::printf("%s%llu", i ? ", " : "", cor_key(from_bits(words[i])));
    std::printf("], \"back\": [");
    for (size_t i = 0; i < words.size(); ++i) {
      const unsigned long long k = cor_key(from_bits(words[i]));
      if (k == NA_KEY) std::printf("%snull", i ? ", " : "");
      else std::printf("%s%llu", i ? ", " : "", bits_of(cor_key_value(k)));
    }
    std::printf("]}\n");
    return 0;
  }
  if (!std::strcmp(argv[1], "taumax")) {
    std::printf("{\"bits\": [");
    for (size_t i = 0; i < words.size(); ++i) std::printf("%s%llu", i ? ", " : "", bits_of(max_taumax_of(words[i])));
    std::printf("]}\n");
    return 0;
  }
  return 2;
}
