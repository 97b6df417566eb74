// k0plan_print.cpp -- prints the pre-pass shape csrc/icikt_k0plan.h chooses, as JSON, for tests/test_k0plan_host.py.
// Host code only: no device header, no library.
//   k0plan_print K0 CUS N COLUMNS [N COLUMNS ...]   K0: the debug plan key (-1: the library's choice); one shape per
//                                                   (N, COLUMNS) couple, and the header's constants
#include <cstdio>
#include <cstdlib>

#include "icikt_k0plan.h"

using namespace icikt::host;

int main(int argc, char** argv) {
  if (argc < 3 || ((argc - 3) & 1)) return 2;
  const int k0 = std::atoi(argv[1]), cus = std::atoi(argv[2]);
  std::printf("{\"large\": %d, \"small\": %d, \"pair\": %d, \"min_rows\": %d, \"max_rows\": %d, \"min_columns_per_cu\": %d, \"shape\": [",
              (int)K0_SHAPE_LARGE, (int)K0_SHAPE_SMALL, (int)K0_SHAPE_PAIR, K0_PAIR_MIN_ROWS, K0_PAIR_MAX_ROWS, K0_PAIR_MIN_COLUMNS_PER_CU);
  for (int a = 3; a + 1 < argc; a += 2)
    std::printf("%s%d", a > 3 ? ", " : "", k0_launch_shape(k0, std::atoll(argv[a]), std::atoll(argv[a + 1]), cus));
  std::printf("]}\n");
  return 0;
}
