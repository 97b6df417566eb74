// icikt_k0plan.h -- which shape of the pre-pass kernel (icikt_prepass.hip) a launch takes, and how many columns of a
// host matrix one launch covers (a chunk of upload_and_prepare, icikt_pipeline.cpp).  Host arithmetic only: no
// device header, so tests/k0plan_print.cpp compiles it with the host compiler alone.  Part of icikt_host.h.
#ifndef ICIKT_K0PLAN_H
#define ICIKT_K0PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace icikt {
namespace host {

// the shapes, as the debug plan key "k0" numbers them (launch_k0's `shape`)
enum : int {
  K0_SHAPE_LARGE = 0,   // 1 024 threads, one workgroup per CU (k0_prepare_large / large8 by the column length)
  K0_SHAPE_SMALL = 1,   // 256 threads: fits beside a running pair kernel; reached through the plan key only
  K0_SHAPE_PAIR = 2,    // 512 threads x 8 elements, two workgroups per CU: two columns in flight
};

// Column lengths at which the 512-thread shape measured faster than the large one in EVERY repeat of the sweep
// (profiles/k0_two_in_flight.log, section 3: 300 .. 50 000 rows at 512, 1 024 and 2 048 columns on 256 CUs): every
// length from 300 to 10 000 rows at every width, by 8 .. 48 %.  At 12 000 and 12 288 rows it lost at 512 and 1 024
// columns, from 14 000 rows on everywhere (by 12 .. 37 %: the 8 192-element tile of the large shape saves these columns
// tiles and a merge level through the scratch).  Outside the range, and at widths the sweep has no point for (fewer
// than two columns per CU), the large shape stays.
constexpr int K0_PAIR_MIN_ROWS = 300;
constexpr int K0_PAIR_MAX_ROWS = 10000;
constexpr int K0_PAIR_MIN_COLUMNS_PER_CU = 2;

// (rows of a column, columns in the launch, CUs of the device) -> shape.  Two columns in flight on a CU pay when the
// launch has columns to spare; a launch of no more columns than CUs is a single round either way, and there the
// 1 024-thread workgroup is the fastest way through ONE column.
inline int k0_pick_shape(int64_t n, int64_t columns, int cus) {
  if (cus <= 0 || columns <= (int64_t)cus) return K0_SHAPE_LARGE;
  if (columns < (int64_t)K0_PAIR_MIN_COLUMNS_PER_CU * cus) return K0_SHAPE_LARGE;   // (not measured)
  if (n < K0_PAIR_MIN_ROWS || n > K0_PAIR_MAX_ROWS) return K0_SHAPE_LARGE;
  return K0_SHAPE_PAIR;
}

// the same under the debug plan key k0 (-1: the library's choice; 0 | 1 | 2 force a shape)
inline int k0_launch_shape(int k0_override, int64_t n, int64_t columns, int cus) {
  if (k0_override == K0_SHAPE_LARGE || k0_override == K0_SHAPE_SMALL || k0_override == K0_SHAPE_PAIR) return k0_override;
  return k0_pick_shape(n, columns, cus);
}

// What runs over the columns of a chunk of a host matrix once they are on the device (upload_and_prepare): the full
// pre-pass (K0), the mask-only one of pairwise_completeness (k0_mask: meta alone must be allocated, mask_alloc), or
// nothing (icikt_pairs_complete_f64 sorts masked copies, not the columns).
enum { kPrepassNone = 0, kPrepassFull = 1, kPrepassMask = 2 };

// how the caller's matrix lies in host memory, as far as the chunk width goes
enum : int {
  K0_VIEW_COL = 0,      // column-major, any element type
  K0_VIEW_ROW = 1,      // row-major: a chunk is n_feat runs of `chunk` cells of elem_bytes each
  K0_VIEW_SPARSE = 2,   // CSC
};
constexpr size_t kRowRunBytes = 512;               // a row-major chunk: runs of at least this many bytes ...
constexpr size_t kRowHalfMax = (size_t)64 << 20;   // ... while a half of the staging blocks stays within this

// Columns of a chunk of upload_and_prepare: what one H2D copy and one pre-pass launch cover (pipelined: one pair-kernel
// launch too) of an n_feat x n_samp matrix (n_feat > 0) on a device of `cus` CUs.  view, elem_bytes: K0_VIEW_*, and the
// bytes of a cell of a row-major view; prepass: kPrepass*; sort_chunk: the columns the sort scratch holds (prepare_alloc).
inline int64_t k0_chunk_columns(int64_t n_feat, int64_t n_samp, int cus, bool pipelined, int view, size_t elem_bytes,
                                int prepass, int sort_chunk) {
  const size_t col_bytes = (size_t)n_feat * sizeof(double);
  // ~8 MB per chunk (an even number of columns: K0 ranges need not be even, but keeps chunks aligned)
  int64_t chunk = std::max<int64_t>(2, (int64_t)(((size_t)8 << 20) / std::max<size_t>(col_bytes, 1)) & ~(int64_t)1);
  // pipelined: a chunk is also what one pre-pass launch and one pair-kernel launch cover.  A pre-pass launch takes
  // the time of ONE column's sort up to a workgroup per CU, so chunks of fewer columns only lengthen the chain of
  // pre-pass launches the last pair-kernel launch waits for (c4: ten chunks of 104 columns finished their pre-pass
  // 1.4 ms after the last copy, four chunks of 256 right behind it)
  if (pipelined) chunk = std::max<int64_t>(chunk, std::min<int64_t>(cus, (n_samp / 4) & ~(int64_t)1));
  // A row-major view gives the chunk as n_feat runs of `chunk` cells, and 8 MB of a tall matrix are few columns (four
  // float64 columns at 262 144 rows: runs of 32 bytes).  The host's packing rate grows with the run up to about 512
  // bytes (DESIGN.md section 11 has the figures), so a row-major chunk is at least that wide where a half of the
  // staging blocks stays within 64 MB.
  if (view == K0_VIEW_ROW) {
    const size_t es = elem_bytes;
    chunk = std::max<int64_t>(chunk, (int64_t)std::min(kRowRunBytes / es, std::max<size_t>(1, kRowHalfMax / ((size_t)n_feat * es))));
  }
  if (prepass == kPrepassFull) chunk = std::min<int64_t>(chunk, std::max(1, sort_chunk));
  return chunk;
}

}  // namespace host
}  // namespace icikt
#endif
