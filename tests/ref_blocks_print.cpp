// ref_blocks_print.cpp -- prints, as one JSON object, what csrc/icikt_blocks.h makes of a query x reference rectangle in
// the layout of a reference that stays prepared (PairBlocks::rect_ref_first: the reference first, the batch behind it),
// the cut cut_rect_rows makes of the same rectangle, and what csrc/icikt_k1plan.h's build_units(np = 2) makes of each
// block's pair list (tests/test_ref_blocks_host.py compiles and runs it; no device, no library):
//   ref_blocks_print SQ SR BUDGET...
//   -> {"query_col": .., "cuts": [{"budget": .., "total": .., "n_blocks": .., "block_max": .., "rows": [[first, last], ..],
//                                 "blocks": [[begin, count, row_first, row_last, [pi..], [pj..], [task words..]], ..]}, ..]}
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icikt_blocks.h"
#include "icikt_k1plan.h"

using namespace icikt::host;

template <typename T>
static void print_ints(const T* v, size_t n) {
  std::printf("[");
  for (size_t q = 0; q < n; ++q) std::printf("%s%lld", q ? ", " : "", (long long)v[q]);
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: ref_blocks_print SQ SR BUDGET...\n");
    return 2;
  }
  const long long Sq = std::atoll(argv[1]), Sr = std::atoll(argv[2]);
  std::printf("{\"query_col\": %lld, \"cuts\": [", (long long)ref_query_col(Sr));
  for (int a = 3; a < argc; ++a) {
    const long long budget = std::atoll(argv[a]);
    PairBlocks pb = PairBlocks::rect_ref_first(Sq, Sr, budget);
    std::printf("%s{\"budget\": %lld, \"total\": %lld, \"n_blocks\": %lld, \"block_max\": %lld, \"rows\": [", a > 3 ? ", " : "",
                budget, (long long)pb.total, (long long)pb.n_blocks, (long long)pb.block_max);
    const auto rows = cut_rect_rows(Sq, Sr, budget);
    for (size_t q = 0; q < rows.size(); ++q) std::printf("%s[%d, %d]", q ? ", " : "", rows[q].first, rows[q].second);
    std::printf("], \"blocks\": [");
    PairBlock b;
    for (bool first = true; pb.next(&b); first = false) {
      std::printf("%s[%lld, %lld, %d, %d, ", first ? "" : ", ", (long long)b.begin, (long long)b.count, b.row_first, b.row_last);
      const size_t n = b.pi ? (size_t)b.count : 0;
      print_ints(b.pi, n);
      std::printf(", ");
      print_ints(b.pj, n);
      std::printf(", ");
      // the task list the pair engine builds of this block: the library hands build_units the same two vectors
      const std::vector<int32_t> pi(b.pi, b.pi + n), pj(b.pj, b.pj + n);
      std::vector<int32_t> units;
      build_units(pi, pj, (int64_t)n, 2, units);
      print_ints(units.data(), units.size());
      std::printf("]");
    }
    std::printf("]}");
  }
  std::printf("]}\n");
  return 0;
}
