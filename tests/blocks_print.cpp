// blocks_print.cpp -- prints, as one JSON object, what csrc/icikt_blocks.h makes of the cases on the command line
// (tests/test_blocks_host.py compiles and runs it; no device, no library):
//   blocks_print rows S BUDGET...             row_offset of every row, and per budget the blocks of PairBlocks::rows
//   blocks_print classes NB BUDGET... CLS...  class_index of the class vector (@S: of no vector, S samples), and per
//                                             budget the slices of PairBlocks::slices
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icikt_blocks.h"

using namespace icikt::host;

template <typename V>
static void print_list(const char* key, const V& v) {
  std::printf("\"%s\": [", key);
  for (size_t q = 0; q < v.size(); ++q) std::printf("%s%lld", q ? ", " : "", (long long)v[q]);
  std::printf("]");
}

// {"budget": .., "total": .., "n_blocks": .., "block_max": .., "blocks": [[begin, count, row_first, row_last, [pi..], [pj..]], ..]}
static void print_blocks(PairBlocks& pb, long long budget) {
  std::printf("{\"budget\": %lld, \"total\": %lld, \"n_blocks\": %lld, \"block_max\": %lld, \"blocks\": [", budget,
              (long long)pb.total, (long long)pb.n_blocks, (long long)pb.block_max);
  PairBlock b;
  for (bool first = true; pb.next(&b); first = false) {
    std::printf("%s[%lld, %lld, %d, %d, [", first ? "" : ", ", (long long)b.begin, (long long)b.count, b.row_first, b.row_last);
    for (int64_t q = 0; b.pi && q < b.count; ++q) std::printf("%s%d", q ? ", " : "", b.pi[q]);
    std::printf("], [");
    for (int64_t q = 0; b.pj && q < b.count; ++q) std::printf("%s%d", q ? ", " : "", b.pj[q]);
    std::printf("]]");
  }
  std::printf("]}");
}

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "rows")) {
    const long long S = std::atoll(argv[2]);
    std::vector<long long> off;
    for (long long i = 0; i < S; ++i) off.push_back(row_offset(S, i));
    std::printf("{");
    print_list("row_offset", off);
    std::printf(", \"cuts\": [");
    for (int a = 3; a < argc; ++a) {
      PairBlocks pb = PairBlocks::rows(S, std::atoll(argv[a]));
      if (a > 3) std::printf(", ");
      print_blocks(pb, std::atoll(argv[a]));
    }
    std::printf("]}\n");
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "classes")) {
    const int nb = std::atoi(argv[2]);
    if (nb < 0 || 3 + nb > argc) return 2;
    std::vector<int32_t> cls;
    for (int a = 3 + nb; a < argc; ++a) cls.push_back(std::atoi(argv[a]));
    const bool none = 3 + nb < argc && argv[3 + nb][0] == '@';   // @S: no class vector, S samples
    const ClassIndex ci = none ? class_index(nullptr, std::atoll(argv[3 + nb] + 1)) : class_index(cls.data(), (int64_t)cls.size());
    std::vector<long long> runs;
    for (const auto& r : ci.runs.run) { runs.push_back(r.first); runs.push_back(r.second); }
    std::printf("{\"total\": %lld, ", (long long)ci.total);
    print_list("pos", ci.pos);
    std::printf(", ");
    print_list("size", ci.size);
    std::printf(", ");
    print_list("base", ci.base);
    std::printf(", ");
    print_list("member", ci.runs.member);
    std::printf(", ");
    print_list("runs", runs);
    std::printf(", \"cuts\": [");
    for (int a = 3; a < 3 + nb; ++a) {
      PairBlocks pb = PairBlocks::slices(&ci.runs, ci.total, std::atoll(argv[a]));
      if (a > 3) std::printf(", ");
      print_blocks(pb, std::atoll(argv[a]));
    }
    std::printf("]}\n");
    return 0;
  }
  std::fprintf(stderr, "usage: blocks_print rows S BUDGET... | classes NB BUDGET... CLS...\n");
  return 2;
}
