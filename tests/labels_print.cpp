// labels_print.cpp -- prints, as one JSON object, what csrc/icikt_labels.h makes of a call's labellings
// (tests/test_labels_host.py compiles and runs it; no device, no library):
//   labels_print plan S N_LAB BYTES_PER_LAB ANOPERMS
//   -> {"batch": .., "groups_max": .., "stage_words": ..}
//   labels_print stage S C N_LAB ANOPERMS WITHIN LABEL...       (N_LAB * S labels, labelling 0 first; anosim's plan)
//   -> {"batch": .., "batches": [{"q0": .., "nb": .., "bad": [q, s, value] | null, "stage": [..], "within": [..]}, ..]}
// Every batch is staged into a buffer of exactly stage_words halfwords filled with 0xFFFF, as the driver would
// (select_labellings), and the run ends at the first bad label; "stage" holds the groups of that batch only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icikt_labels.h"

using namespace icikt::host;

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "plan")) {
    const LabelBatches p = label_batches(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]));
    std::printf("{\"batch\": %lld, \"groups_max\": %lld, \"stage_words\": %llu}\n", (long long)p.batch, (long long)p.groups_max,
                (unsigned long long)p.stage_words);
    return 0;
  }
  if (argc < 7 || std::strcmp(argv[1], "stage")) {
    std::fprintf(stderr, "usage: labels_print plan S N_LAB BYTES_PER_LAB ANOPERMS | stage S C N_LAB ANOPERMS WITHIN LABEL...\n");
    return 2;
  }
  const long long S = std::atoll(argv[2]), C = std::atoll(argv[3]), n_lab = std::atoll(argv[4]);
  const bool want_within = std::atoi(argv[6]) != 0;
  if (argc != 7 + n_lab * S) {
    std::fprintf(stderr, "labels_print: %lld labels expected\n", n_lab * S);
    return 2;
  }
  std::vector<int32_t> labels;
  for (int a = 7; a < argc; ++a) labels.push_back((int32_t)std::atol(argv[a]));
  const int32_t* obs = labels.data();
  const int32_t* perm_cls = labels.data() + S;   // (never read when n_lab == 1)
  const LabelBatches p = label_batches(S, n_lab, 2 * S, std::atoll(argv[5]));
  std::vector<uint16_t> stage(p.stage_words);
  std::vector<int64_t> size_of((size_t)C, 0), within((size_t)p.batch, -1);
  std::printf("{\"batch\": %lld, \"batches\": [", (long long)p.batch);
  for (long long q0 = 0; q0 < n_lab; q0 += p.batch) {
    const long long nb = std::min<long long>(p.batch, n_lab - q0);
    stage.assign(p.stage_words, 0xFFFF);
    const BadLabel bad = stage_labellings(obs, perm_cls, S, C, q0, nb, stage.data(), want_within ? within.data() : nullptr,
                                          want_within ? size_of.data() : nullptr);
    std::printf("%s{\"q0\": %lld, \"nb\": %lld, \"bad\": ", q0 ? ", " : "", q0, nb);
    if (bad.q >= 0) std::printf("[%lld, %lld, %d]", (long long)bad.q, (long long)bad.s, (int)bad.value);
    else std::printf("null");
    std::printf(", \"stage\": [");
    const size_t words = (size_t)((nb + icikt::ANO_PB - 1) / icikt::ANO_PB) * (size_t)S * icikt::ANO_PB;
    for (size_t w = 0; w < words; ++w) std::printf("%s%u", w ? ", " : "", (unsigned)stage[w]);
    std::printf("], \"within\": [");
    for (long long l = 0; want_within && bad.q < 0 && l < nb; ++l) std::printf("%s%lld", l ? ", " : "", (long long)within[(size_t)l]);
    std::printf("]}");
    for (long long k = 0; k < C; ++k)
      if (size_of[(size_t)k] != 0) {
        std::fprintf(stderr, "labels_print: size_of is not zero on return\n");
        return 1;
      }
    if (bad.q >= 0) break;
  }
  std::printf("]}\n");
  return 0;
}
