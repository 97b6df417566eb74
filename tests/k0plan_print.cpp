// k0plan_print.cpp -- prints what csrc/icikt_k0plan.h decides, as JSON, for tests/test_k0plan_host.py.
// Host code only: no device header, no library.
//   k0plan_print K0 CUS N COLUMNS [N COLUMNS ...]   K0: the debug plan key (-1: the library's choice); one shape per
//                                                   (N, COLUMNS) couple, and the header's constants
//   k0plan_print chunk                              the columns of a chunk (k0_chunk_columns), one per case of standard
//                                                   input: N_FEAT N_SAMP CUS PIPELINED VIEW ELEM_BYTES PREPASS SORT_CHUNK
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "icikt_k0plan.h"

using namespace icikt::host;

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "chunk")) {
    long long n_feat, n_samp;
    int cus, pipelined, view, es, prepass, sort_chunk;
    std::printf("[");
    for (int k = 0; std::cin >> n_feat >> n_samp >> cus >> pipelined >> view >> es >> prepass >> sort_chunk; ++k)
      std::printf("%s%lld", k ? ", " : "",
                  (long long)k0_chunk_columns(n_feat, n_samp, cus, pipelined != 0, view, (size_t)es, prepass, sort_chunk));
    std::printf("]\n");
    return std::cin.eof() ? 0 : 2;
  }
  if (argc < 3 || ((argc - 3) & 1)) return 2;
  const int k0 = std::atoi(argv[1]), cus = std::atoi(argv[2]);
  std::printf("{\"large\": %d, \"small\": %d, \"pair\": %d, \"min_rows\": %d, \"max_rows\": %d, \"min_columns_per_cu\": %d, \"shape\": [",
              (int)K0_SHAPE_LARGE, (int)K0_SHAPE_SMALL, (int)K0_SHAPE_PAIR, K0_PAIR_MIN_ROWS, K0_PAIR_MAX_ROWS, K0_PAIR_MIN_COLUMNS_PER_CU);
  for (int a = 3; a + 1 < argc; a += 2)
    std::printf("%s%d", a > 3 ? ", " : "", k0_launch_shape(k0, std::atoll(argv[a]), std::atoll(argv[a + 1]), cus));
  std::printf("]}\n");
  return 0;
}
