// icikt_blocks.h -- which pairs a selection entry (icikt_topk_*, icikt_edges_*, icikt_class_medians_*,
// icikt_class_matrix_*, icikt_quantiles_*, icikt_padjust_*, icikt_mst_*, icikt_anosim_*, icikt_hclust_*) computes, and
// in which blocks: whole rows of the combn triangle (all nine), or slices of the within-class pair list
// (icikt_class_medians_* with several classes), or whole query rows of the query x reference rectangle (icikt_cross_*).
// Plain C++, no device header: tests/test_blocks_host.py and tests/test_cross_blocks_host.py compile it alone.  Host
// memory is O(S) for the classes and O(block) for a slice or a run of rectangle rows.
#ifndef ICIKT_BLOCKS_H
#define ICIKT_BLOCKS_H

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace icikt {
namespace host {

// Pairs of a block when no tkblock key says otherwise.  2^24 pairs fill the chip (256 CUs x at most 32 waves x 2
// pairs: 16 384 pairs in flight) a thousand times over, so a block's launch tail is lost in its body, and the buffers
// of a block -- out4 32 B, the pair kernel's counts 24, pi / pj 8, the task list 8, reasons 4 per pair, a ninth on top
// for the buffers' growth margin -- stay at 1.4 GB.  The whole triangle of up to 5 793 columns is ONE block.
constexpr int64_t kTriangleBlockPairs = (int64_t)1 << 24;
// first pair of row i of combn(S, 2)
inline int64_t row_offset(int64_t S, int64_t i) { return i * (2 * S - i - 1) / 2; }
// rows [a, b) of the combn triangle per block: the largest run from a within the budget, at least one row; a run of
// several rows ends on an even row (the next block then starts on one: the pair kernel's tasks pair the rows 2a, 2a + 1)
inline std::vector<std::pair<int, int>> cut_rows(int64_t S, int64_t budget) {
  std::vector<std::pair<int, int>> blocks;
  int64_t a = 0;
  while (a < S - 1) {
    int64_t b = a, pairs = 0;
    while (b < S - 1 && (b == a || pairs + (S - 1 - b) <= budget)) { pairs += S - 1 - b; ++b; }
    if (b < S - 1 && (b & 1) && b - a >= 2) --b;
    blocks.emplace_back((int)a, (int)b);
    a = b;
  }
  return blocks;
}

// query rows [a, b) of the Sq x Sr rectangle per block (Sr pairs a row): the largest run from a within the budget, at
// least one row; a run of several rows ends on an even row, for cut_rows' reason
inline std::vector<std::pair<int, int>> cut_rect_rows(int64_t Sq, int64_t Sr, int64_t budget) {
  std::vector<std::pair<int, int>> blocks;
  if (Sr <= 0) return blocks;
  const int64_t fit = std::max<int64_t>(1, budget / Sr);
  int64_t a = 0;
  while (a < Sq) {
    int64_t b = std::min(Sq, a + fit);
    if (b < Sq && (b & 1) && b - a >= 2) --b;
    blocks.emplace_back((int)a, (int)b);
    a = b;
  }
  return blocks;
}
// the device column of reference column 0: the query columns come first, and the reference starts on an even column
// (the pre-pass's tables are interleaved in blocks of two columns), behind one padding column when Sq is odd
inline int64_t rect_ref_col(int64_t Sq) { return Sq + (Sq & 1); }
// the mirror layout of a reference that stays prepared (icikt_ref_*): the reference columns come first, and the query
// batch starts on an even column, behind one padding column when Sr is odd -- the device column of query column 0
inline int64_t ref_query_col(int64_t Sr) { return Sr + (Sr & 1); }

// the members of the classes, class by class in class-index order, ascending sample index inside a class
struct ClassRuns {
  std::vector<int32_t> member;                  // [S] sample indices
  std::vector<std::pair<int32_t, int32_t>> run; // per non-empty class: [first, last) of `member`
};

// the pairs of the call's order from a cursor on: class `ci`, pair (a, b) of its members
struct PairCursor {
  size_t ci = 0;
  int32_t a = 0, b = 1;
};

// up to `budget` pairs from the cursor on into pi / pj (sample indices); the cursor moves behind them
inline void next_slice(const ClassRuns& cr, PairCursor* cur, int64_t budget, std::vector<int32_t>* pi, std::vector<int32_t>* pj) {
  pi->clear();
  pj->clear();
  while (cur->ci < cr.run.size() && (int64_t)pi->size() < budget) {
    const int32_t first = cr.run[cur->ci].first, m = cr.run[cur->ci].second - first;
    if (cur->a >= m - 1) {   // the class is through (a singleton has no pair)
      ++cur->ci;
      cur->a = 0;
      cur->b = 1;
      continue;
    }
    const int64_t take = std::min<int64_t>(m - cur->b, budget - (int64_t)pi->size());
    const int32_t sa = cr.member[first + cur->a];
    for (int64_t q = 0; q < take; ++q) {
      pi->push_back(sa);
      pj->push_back(cr.member[first + cur->b + q]);
    }
    cur->b += (int32_t)take;
    if (cur->b >= m) {
      ++cur->a;
      cur->b = cur->a + 1;
    }
  }
}

// the classes of a call, O(S) whatever n_class is: the runs, and per sample its position in its class, the class's
// size and the class's first pair in the call's order (the device's MedianClasses); total: the within-class pairs
struct ClassIndex {
  ClassRuns runs;
  std::vector<int32_t> pos, size;
  std::vector<long long> base;
  int64_t total = 0;
};
// cls: a class index per sample, or null for one class of all S samples
inline ClassIndex class_index(const int32_t* cls, int64_t S) {
  ClassIndex ci;
  ClassRuns& cr = ci.runs;
  cr.member.resize((size_t)S);
  std::iota(cr.member.begin(), cr.member.end(), 0);
  if (cls) std::stable_sort(cr.member.begin(), cr.member.end(), [cls](int32_t a, int32_t b) { return cls[a] < cls[b]; });
  ci.pos.resize((size_t)S);
  ci.size.resize((size_t)S);
  ci.base.resize((size_t)S);
  for (int64_t f = 0; f < S;) {
    int64_t l = f + 1;
    while (cls && l < S && cls[cr.member[l]] == cls[cr.member[f]]) ++l;
    if (!cls) l = S;
    cr.run.emplace_back((int32_t)f, (int32_t)l);
    const int64_t m = l - f;
    for (int64_t q = f; q < l; ++q) {
      const int32_t s = cr.member[q];
      ci.pos[s] = (int32_t)(q - f);
      ci.size[s] = (int32_t)m;
      ci.base[s] = (long long)ci.total;
    }
    ci.total += m * (m - 1) / 2;
    f = l;
  }
  return ci;
}

// one block of a call: pairs [begin, begin + count) of the call's pair order -- rows [row_first, row_last) of the
// combn triangle, or (pi != null) a slice of the class list as sample indices, or (pi != null, row_last > row_first)
// query rows [row_first, row_last) of the rectangle as device columns (either layout); pi / pj are valid until the next block is asked for
struct PairBlock {
  int64_t begin = 0, count = 0;
  int row_first = 0, row_last = 0;
  const int32_t *pi = nullptr, *pj = nullptr;
};

// a call's blocks in order
class PairBlocks {
 public:
  // whole rows of combn(S, 2), `budget` pairs per block of several rows (cut_rows)
  static PairBlocks rows(int64_t S, int64_t budget) {
    PairBlocks p;
    p.S = S;
    p.total = S * (S - 1) / 2;
    p.rows_ = cut_rows(S, budget);
    p.n_blocks = (int64_t)p.rows_.size();
    for (const auto& b : p.rows_) p.block_max = std::max(p.block_max, row_offset(S, b.second) - row_offset(S, b.first));
    return p;
  }
  // slices of the classes' pair list (`total` pairs, class_index), each but the last of `budget` pairs and of 2^30 at
  // most (a pair list holds fewer than 2^31 - 1); cr must outlive the blocks
  static PairBlocks slices(const ClassRuns* cr, int64_t total, int64_t budget) {
    PairBlocks p;
    p.cr_ = cr;
    p.total = total;
    p.budget_ = std::min<int64_t>(budget, (int64_t)1 << 30);
    p.n_blocks = (total + p.budget_ - 1) / p.budget_;
    p.block_max = std::max<int64_t>(1, std::min(total, p.budget_));
    return p;
  }
  // whole query rows of the Sq x Sr rectangle, pair p = q * Sr + r of the call's order, `budget` pairs (2^30 at most)
  // per block of several rows (cut_rect_rows).  A block's pi / pj are (q, rect_ref_col(Sq) + r), generated into the
  // block's host vectors as next() is called: sorted by (pi, pj), so the task list pairs the rows 2a and 2a + 1 over
  // every reference column (build_units' sorted branch)
  static PairBlocks rect(int64_t Sq, int64_t Sr, int64_t budget) {
    PairBlocks p;
    p.rect_ = true;
    p.Sq_ = Sq;
    p.Sr_ = Sr;
    p.total = Sq * Sr;
    p.rows_ = cut_rect_rows(Sq, Sr, std::min<int64_t>(budget, (int64_t)1 << 30));
    p.n_blocks = (int64_t)p.rows_.size();
    for (const auto& b : p.rows_) p.block_max = std::max(p.block_max, (int64_t)(b.second - b.first) * Sr);
    return p;
  }
  // the same rectangle, the same cut and the same pair order over the mirror layout (the reference first, icikt_ref_*):
  // a block's pi / pj are (ref_query_col(Sr) + q, r) -- the query is still the first column of a pair and the list is
  // still sorted by (pi, pj), with pi > pj
  static PairBlocks rect_ref_first(int64_t Sq, int64_t Sr, int64_t budget) {
    PairBlocks p = rect(Sq, Sr, budget);
    p.ref_first_ = true;
    return p;
  }
  int64_t S = 0, total = 0, n_blocks = 0, block_max = 1;   // S: of rows(); block_max: the largest block's pairs (at least 1)
  // the next block into *b; false behind the last one
  bool next(PairBlock* b) {
    if (at_ >= n_blocks) return false;
    if (cr_) {
      next_slice(*cr_, &cur_, budget_, &pi_, &pj_);
      *b = PairBlock{done_, (int64_t)pi_.size(), 0, 0, pi_.data(), pj_.data()};
    } else if (rect_) {
      const int first = rows_[at_].first, last = rows_[at_].second;
      const size_t count = (size_t)(last - first) * (size_t)Sr_;
      const int32_t row0 = ref_first_ ? (int32_t)ref_query_col(Sr_) : 0, col0 = ref_first_ ? 0 : (int32_t)rect_ref_col(Sq_);
      pi_.resize(count);
      pj_.resize(count);
      size_t p = 0;
      for (int q = first; q < last; ++q)
        for (int32_t r = 0; r < (int32_t)Sr_; ++r, ++p) {
          pi_[p] = row0 + (int32_t)q;
          pj_[p] = col0 + r;
        }
      *b = PairBlock{(int64_t)first * Sr_, (int64_t)count, first, last, pi_.data(), pj_.data()};
    } else {
      const int first = rows_[at_].first, last = rows_[at_].second;
      *b = PairBlock{row_offset(S, first), row_offset(S, last) - row_offset(S, first), first, last, nullptr, nullptr};
    }
    done_ = b->begin + b->count;
    ++at_;
    return true;
  }

 private:
  std::vector<std::pair<int, int>> rows_;
  const ClassRuns* cr_ = nullptr;
  PairCursor cur_;
  bool rect_ = false, ref_first_ = false;
  int64_t Sq_ = 0, Sr_ = 0;
  int64_t budget_ = 0, at_ = 0, done_ = 0;
  std::vector<int32_t> pi_, pj_;
};

}  // namespace host
}  // namespace icikt
#endif
