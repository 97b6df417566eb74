// icikt_labels.h -- the labellings of the permutation-test entries (icikt_anosim_*, icikt_permanova_*) as far as they
// need no device: the one test of a label's range (label_in_range; every entry with a cls argument makes it through it),
// how many labellings an upload takes, and how a batch of them is checked and laid out for the permutation kernels.
// Plain C++, no device header: tests/test_labels_host.py compiles it alone.  The driver that moves the batches is
// select_labellings (icikt_capi_select.cpp).
#ifndef ICIKT_LABELS_H
#define ICIKT_LABELS_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace icikt {

constexpr int ANO_PB = 16;                          // labellings a workgroup of the permutation kernel takes side by side
constexpr long long ANO_PERMS_MAX = 1 << 20;        // labellings per upload (anoperms)
constexpr long long ANO_BATCH_BYTES = 64ll << 20;   // ... and the bytes an upload's labellings cost when no key says otherwise

namespace host {

// a label's range, tested here and nowhere else
inline bool label_in_range(int32_t v, int64_t n_class) { return v >= 0 && v < n_class; }
// the first s with lab[s] outside [0, n_class); n when every label is inside
inline int64_t first_bad_label(const int32_t* lab, int64_t n, int64_t n_class) {
  for (int64_t s = 0; s < n; ++s)
    if (!label_in_range(lab[s], n_class)) return s;
  return n;
}

// Labellings per upload of a call with n_lab of them over S samples: the anoperms plan key (> 0), else what
// ANO_BATCH_BYTES hold at bytes_per_lab a labelling (anosim: the 2 S bytes of its labels; permanova: the largest of
// labels, column sums and bins, 16 max(S, n_class)) in whole groups of ANO_PB, at least one group; either way at most
// ANO_PERMS_MAX and n_lab.  groups_max and stage_words are the groups and the halfwords of a full batch.
struct LabelBatches {
  int64_t batch, groups_max;
  size_t stage_words;
};
inline LabelBatches label_batches(int64_t S, int64_t n_lab, int64_t bytes_per_lab, long long anoperms) {
  constexpr int PB = ANO_PB;
  int64_t batch = anoperms > 0 ? (int64_t)anoperms : std::max<int64_t>(PB, ANO_BATCH_BYTES / bytes_per_lab / PB * PB);
  batch = std::min<int64_t>(std::min<int64_t>(batch, ANO_PERMS_MAX), n_lab);
  const int64_t groups_max = (batch + PB - 1) / PB;
  return {batch, groups_max, (size_t)groups_max * (size_t)S * PB};
}

// a label out of range: sample s of labelling q holds value (q < 0: none)
struct BadLabel {
  int64_t q = -1, s = 0;
  int32_t value = 0;
};

// Labellings [q0, q0 + nb) of a call -- 0 is obs, q >= 1 row q - 1 of perm_cls [.][S] -- checked in that order and laid
// out as the device takes them, [groups][S][ANO_PB] halfwords: labelling q0 + l gives sample s the class
// stage[(l / PB) S PB + s PB + l % PB]; the unused slots of the last group are labelling 0s, their sums ignored.
// Returns the first bad label: the labellings before it are staged, no labelling behind it is touched.  within
// (optional, [nb]): per labelling the pairs of samples that share a class, the sum over the classes of C(size, 2); it
// needs size_of [n_class], zero on entry and on return.  One pass over a labelling: a call of one batch stages all its
// labels before anything runs beside it, and a second pass over them shows in its wall time.
inline BadLabel stage_labellings(const int32_t* obs, const int32_t* perm_cls, int64_t S, int64_t n_class, int64_t q0,
                                 int64_t nb, uint16_t* stage, int64_t* within = nullptr, int64_t* size_of = nullptr) {
  constexpr int PB = ANO_PB;
  for (int64_t l = 0; l < nb; ++l) {
    const int64_t q = q0 + l;
    const int32_t* lab = q == 0 ? obs : perm_cls + (size_t)(q - 1) * (size_t)S;
    uint16_t* out = stage + (size_t)(l / PB) * (size_t)S * PB + (size_t)(l % PB);
    int64_t s = 0, w = 0;
    if (within) {
      for (; s < S && label_in_range(lab[s], n_class); ++s) {
        out[(size_t)s * PB] = (uint16_t)lab[s];
        w += size_of[(size_t)lab[s]]++;
      }
      for (int64_t t = 0; t < s; ++t) size_of[(size_t)lab[t]] = 0;
      within[l] = w;
    } else {
      for (; s < S && label_in_range(lab[s], n_class); ++s) out[(size_t)s * PB] = (uint16_t)lab[s];
    }
    if (s < S) return {q, s, lab[s]};
  }
  for (int64_t l = nb; l < (nb + PB - 1) / PB * PB; ++l) {
    uint16_t* out = stage + (size_t)(l / PB) * (size_t)S * PB + (size_t)(l % PB);
    for (int64_t s = 0; s < S; ++s) out[(size_t)s * PB] = 0;
  }
  return {};
}

}  // namespace host
}  // namespace icikt
#endif
