// icikt_device.h -- structures, layouts and launcher declarations shared by the device units (icikt_prepass.hip,
// icikt_kernels.hip, icikt_epilogue.hip, icikt_cor.hip, icikt_diag.hip, icikt_topk.hip, icikt_edges.hip, icikt_medians.hip, icikt_quantiles.hip, icikt_classmat.hip, icikt_padjust.hip, icikt_mst.hip, icikt_hclust.hip, icikt_anosim.hip, icikt_permanova.hip, icikt_permdisp.hip, icikt_cross.hip) and the C-ABI
// host side (icikt_capi*.cpp, icikt_multi.cpp).  Internal; the public boundary is include/icikt.h.
#ifndef ICIKT_DEVICE_H
#define ICIKT_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icikt_k1plan.h"   // ColStats, and the pair kernel's LDS layout and option word (K1_*, k1_*, ICIKT_CNT_BYTES)
#include "icikt_labels.h"   // ANO_PB, ANO_PERMS_MAX, ANO_BATCH_BYTES: the label plane and its batches

namespace icikt {

constexpr int ICIKT_PERSPECTIVE_LOCAL_ = 0;  // == ICIKT_PERSPECTIVE_LOCAL
constexpr int ICIKT_CNT_FIELDS_ = 11;        // == ICIKT_CNT_FIELDS

constexpr int COL_ODD_TIE = 1;   // ColStats::flags
__host__ __device__ inline uint32_t col_stream_cost(const ColStats& st) { return (uint32_t)st.flags >> 8; }

// tie-program entry: rows of the step | kind << 7 | closes << 9 | n0 << 10 (MIXED: rows of its first sub-step)
constexpr uint32_t TPROG_KIND_HOT = 0u, TPROG_KIND_MIXED = 1u, TPROG_KIND_GROUP = 2u, TPROG_KIND_SOLO = 3u;
__host__ __device__ inline uint32_t tprog_rows(uint32_t e) { return e & 127u; }
__host__ __device__ inline uint32_t tprog_kind(uint32_t e) { return (e >> 7) & 3u; }
__host__ __device__ inline bool tprog_closes(uint32_t e) { return ((e >> 9) & 1u) != 0u; }
__host__ __device__ inline uint32_t tprog_n0(uint32_t e) { return (e >> 10) & 63u; }
// What the generator (k0_tie_program, icikt_prepass.hip) and the pair kernel that walks the program (k1_pairs) must agree on:
constexpr int TPROG_KS = 32;   // == k1_ks(true): MIXED steps take groups of up to this many rows
constexpr int TPROG_WIN = 16384, TPROG_LIST = 1024;   // positions of a generator window; steps listed per window
constexpr int TPROG_MARKS = 4;   // segment marks written behind the program (prog_tail: positions, then their steps)

// setup_missing_matrix (R/utils.R:1-23) on the device: which cells of the data matrix are excluded (become NA,
// R/kendalltau.R:119-121) before the pre-pass.  The pre-pass applies it while it reads the matrix, so the masked copy
// `exclude_data` never exists.  A NaN in the data is missing for ici_kt whether or not NaN is in global_na
// (Rcpp is_na, src/kendallc.cpp:181), but counts as excluded (n_good, keep) only when it is.
constexpr int ICIKT_MASK_VALS = 32;   // distinct finite global_na values the device rule holds (the struct travels as a kernel
                                      // argument); a longer list is masked by the host front-end before the call (api.py, icikt_mi355x.R)
struct MaskSpec {
  int mask_nan;                  // global_na holds NA
  int mask_inf;                  // global_na holds Inf: is.infinite(), both signs
  int n_vals;                    // the other global_na values, compared with ==
  double vals[ICIKT_MASK_VALS];
};
__host__ __device__ inline bool mask_excluded(const MaskSpec& ms, double v) {
  bool ex = (ms.mask_nan && v != v) || (ms.mask_inf && (v - v != 0.0) && v == v);   // v - v: NaN for +-Inf, 0 otherwise
  for (int k = 0; k < ms.n_vals; ++k) ex = ex || (v == ms.vals[k]);   // (n_vals <= ICIKT_MASK_VALS, wave-uniform)
  return ex;
}

// Per-pair integers produced by K1 for the global perspective.
struct PairRaw {
  unsigned long long dis;   // #{(i,j): x_i < x_j, y_i > y_j}
  unsigned long long ntie;  // #{i<j: x_i == x_j, y_i == y_j}
  uint32_t c_both;          // rows missing in both columns
  uint32_t g;               // rows in both fill groups (== c_both unless fl(min-0.1) == min)
};

constexpr int K1_CNT_MIN_GROUPS = 8;        // columns too long for the half-wave kernels: girow is written, and count mode used, above this many tie groups
constexpr uint16_t GIROW_NONE = 0xFFFFu;   // PrepView::girow: the row is its own tie group

// Device pointers + sizes of the prepared matrix (HBM layout).
static_assert(sizeof(ColStats) == 72, "ColStats is 9 words of a column's meta record");

struct PrepView {
  int n;       // n_feat (rows per column)
  int n_pad;   // n rounded up to a multiple of 64
  int n_ord;   // n_pad + 256: stride of `order`, zero padded so that K1 can load rows three steps ahead
  int W;       // ceil(n / 64) bitset words
  int Wp;      // W + 1 (one zero guard word)
  int npow2;   // sort scratch length per column
  int n_samp;
  // per column, stride n_pad
  uint16_t* order;   // [S][n_ord]  row at processing position k (descending value)
  uint32_t* order_w; // [S][n_ord]  the same as 32-bit words, for columns too long for the half-wave kernels (else nullptr): the whole-wave
                     //              kernels reload their ring of rows from it after a step of fewer than 64 rows (k1_pairs)
  int rec_rows;      // rows of a rec / hirow block: n_pad + 8.  Row n_pad is the GUARD ROW of every column: q = n_pad (a
                     // position in the guard word of a pair kernel's bitset), lo = 0, hi = 0 -- the empty lanes of a step
                     // of the tie program name it (srow below), so that they gather "a row that never counts, is never
                     // counted, queries 0 and inserts a bit no query reaches" without an instruction of their own
  uint32_t* rec;     // [S/2][rec_rows][2]  per row: q | lo << 16  (ascending stable position, group start),
                     // the columns 2a and 2a+1 interleaved: one 8-byte gather per row serves both
  uint16_t* hirow;   // [S/2][rec_rows][2]  per row: last ascending position of its tie group, the columns 2a and 2a+1
                     // interleaved like rec (a half-wave GROUP step reads both pairs' ends with one 4-byte gather per row)
  uint16_t* girow;   // [S/2][rec_rows][2]  per row: the place of its tie group in the column's list `tgroups` (groups of
                     // >= 2 rows, ascending), GIROW_NONE for a row that is its own group; interleaved like hirow.  A half-
                     // wave GROUP step counts the streamed group's rows per tie group of the gathered column in a table of
                     // counters indexed by it (count mode, k1_pairs)
  // per column, stride Wp
  // per column one record of mstride = 3 * Wp + 9 words (one array: one collective moves it between ranks):
  //   [Wp] mask      missing rows
  //   [Wp] fillmask  rows in the fill group
  //   [Wp] gflag     bit k: processing position k starts a tie group
  //   [9]  ColStats
  unsigned long long* meta;
  int mstride;
  __host__ __device__ unsigned long long* col_mask(int c) const { return meta + (int64_t)c * mstride; }
  __host__ __device__ unsigned long long* col_fillmask(int c) const { return meta + (int64_t)c * mstride + Wp; }
  __host__ __device__ unsigned long long* col_gflag(int c) const { return meta + (int64_t)c * mstride + 2 * Wp; }
  __host__ __device__ ColStats* col_stats(int c) const {
    return reinterpret_cast<ColStats*>(meta + (int64_t)c * mstride + 3 * Wp);
  }
  uint32_t* tgroups;             // [S][tg_stride] tie groups (size >= 2), ascending: lo | hi << 16
  int tg_stride;                 // n_pad / 2 + 1
  // The tie program of a column as the STREAMED side of a half-wave kernel (n <= 30 656): the steps the pair kernel
  // takes from where the column's tie groups begin, cut and classified ONCE per column by the pre-pass instead of by
  // every one of its S - 1 pairs (k0_tie_program; entry layout: TPROG_*).  Round 4, second half: a step comes with its RECORD --
  //   srow   the rows of the step in the LANE LAYOUT the pair kernel runs it in, 64 entries whatever the step holds
  //          (HOT / GROUP: lane = row of the step; MIXED: lanes 0..31 the first sub-step, lanes 32..63 the second);
  //          an empty lane names the guard row (rec_rows above).  The pair kernel reads them three steps ahead like the
  //          rows of the singleton region: no step re-lays its rows out, rotates its ring or selects guard values;
  //   smask  MIXED steps: per lane l = 0..31 which flags of the pair kernel's two in-step compare vectors (x: vector 1,
  //          y: vector 2; both sub-steps of the lane) belong to pairs INSIDE a tie group.
  // Three guard steps (guard rows only) follow a column's last step: what the pair kernel loads ahead.  All of it is a
  // function of order and gflag: rebuilt, not exchanged, between ranks.
  uint32_t* tprog;               // [S][tp_stride]; tp_stride = n_pad + 2 (a step takes at least one row; 0 ends the list)
  int tp_stride;
  int sr_steps;                  // records per column: n_pad / 17 + 8 (two consecutive steps hold >= 34 rows, see k0_tie_program)
  uint16_t* srow;                // [S][sr_steps][64]
  uint2* smask;                  // [S][sr_steps][32]
  // sort scratch (per column of the current chunk)
  unsigned long long* sort_keys;  // [chunk][npow2]
  uint32_t* sort_idx;             // [chunk][npow2]
  // ---- wide columns (65 535 < n <= ICIKT_MAX_FEATURES_WIDE): 32-bit positions, separate arrays, a plain pair
  // kernel (k1_wide).  order / rec / hirow / tgroups are not allocated then.
  int wide;
  uint32_t* order32;              // [S][n_pad]  row at processing position k (descending value)
  uint32_t* q32;                  // [S][n_pad]  per row: ascending stable position
  uint32_t* lo32;                 // [S][n_pad]  per row: first position of its tie group
  uint32_t* hi32;                 // [S][n_pad]  per row: last position of its tie group
  unsigned long long* k0_bits;    // [chunk][2][Wp + 1]  K0's group-start and fill bitsets (LDS holds them up to 65 535 rows)
};

// ms: cells to exclude while reading dX (nullptr: NaN = missing, nothing else); keep: optional [n_samp][n] bytes,
// 1 = not excluded (the reference's `keep = t(!exclude_loc)`, R/kendalltau.R:417)
// shape (the same results from each; icikt_k0plan.h picks): 0 the 1 024-thread workgroups, one per CU; 1 256-thread
// workgroups (4 waves per column) that fit a CU beside a running pair kernel; 2 512-thread workgroups, two per CU
hipError_t launch_k0(const PrepView& pv, const double* dX, int64_t ld, int col_begin, int ncols, const MaskSpec* ms,
                     uint8_t* keep, int shape, hipStream_t s);
// Full-matrix assembly (scale_and_reshape, R/kendalltau.R:357-421) on the device.
//   launch_out_stats: red[0] = max(taumax) over the pairs, NaN skipped, as a sortable key (0 = none); red[1..5] =
//     pairs per reason code; red[6] = max(n_good)
//   launch_assemble:  five S x S matrices (cor, raw, pvalue, taumax, completeness), symmetric, diagonal rows
// pi / pj == nullptr: pair p is pair `first + p` of combn(S, 2) order.  n_good == nullptr: n - ColStats::nexcl.
hipError_t launch_out_stats(const PrepView& pv, const double* out4, const int32_t* reasons, int64_t n_pairs,
                            const int64_t* n_good, unsigned long long* red, hipStream_t s);
hipError_t launch_assemble(const PrepView& pv, const double* out4, const int32_t* pi, const int32_t* pj, int64_t n_pairs,
                           const int64_t* n_good, const unsigned long long* red, int scale_max, int diag_good,
                           double* out5, hipStream_t s);
// launch_out_stats without the zeroing of red: the statistics of one more block of pairs are added to what red holds
// (icikt_topk_f64 runs the triangle in blocks; the caller zeroes red's 8 words before the first)
hipError_t launch_out_stats_accum(const PrepView& pv, const double* out4, const int32_t* reasons, int64_t n_pairs,
                                  unsigned long long* red, hipStream_t s);
// ---- top-k partners per sample (icikt_topk.hip) ----
// Every column's running list of its k best partners, twice (cur[c] says which copy is current; a merge writes the
// other one and flips it): keys as dbl_sortable gives them, partner columns, and the four out4 doubles of each entry.
struct TopkLists {
  unsigned long long* key;   // [2][S][k]
  int32_t* partner;          // [2][S][k]
  double* vals;              // [2][S][k][4]: raw, pvalue, taumax, completeness
  int32_t* count;            // [S] entries of the current list (zeroed before the first merge)
  int32_t* cur;              // [S] 0 | 1 (zeroed likewise)
  int k;                     // 1 .. ICIKT_TOPK_MAX
};
// out4: the records of the pairs of rows [row_a, row_b) of combn(S, 2), in combn order (row_b <= S - 1, S <= 65 535)
hipError_t launch_topk_merge(const TopkLists& L, const double* out4, int S, int row_a, int row_b, hipStream_t s);
// idx [S][k] (-1 padded), out5k [5][S][k] (NA_real_ padded), n_valid [S] (may be null); red: launch_out_stats' record
hipError_t launch_topk_finish(const TopkLists& L, const unsigned long long* red, int S, int scale_max, int32_t* idx,
                              double* out5k, int32_t* n_valid, hipStream_t s);
// ---- query x reference rectangle (icikt_cross.hip) ----
// out4: the records of query rows [row_first, row_first + n_rows) of the Sq x Sr rectangle, query-major.  Writes the
// rows' final lists: idx [Sq][k] (-1 padded), planes 1 .. 4 of planes [5][Sq][k] (NA_real_ padded), n_valid [Sq].
hipError_t launch_cross_topk(const double* out4, int Sr, int k, int row_first, int n_rows, long long Sq, int32_t* idx,
                             double* planes, int32_t* n_valid, hipStream_t s);
// out4: the records of pairs [begin, begin + count) of the rectangle's P pairs -> planes 1 .. 4 of planes [5][P]
hipError_t launch_cross_planes(const double* out4, long long count, long long begin, long long P, double* planes,
                               hipStream_t s);
// plane 0 (cor) of planes [5][P] from plane 1 (raw) and red, launch_out_stats' record, once it is final; idx (may be
// null): [P], a negative entry marks a padding slot (NA_real_)
hipError_t launch_cross_cor(const unsigned long long* red, int scale_max, const int32_t* idx, long long P, double* planes,
                            hipStream_t s);
// n cells of NaN: the padding column behind an odd number of query columns
hipError_t launch_cross_pad(double* col, int n, hipStream_t s);
// The class fold of a labelled reference.  out4: the records of query rows [row_first, row_first + n_rows), as
// launch_cross_topk takes them; member [Sr]: the reference columns sorted stably by class; first [n_class + 1]: class c
// is member[first[c] .. first[c + 1]).  Leaves every (row, class) cell's two middle keys in med2 [2][n_class][Sq] and
// its partners in n_valid [n_class][Sq]; stage as launch_median_select takes it.  launch_cross_class_cor, once red
// (launch_out_stats' record) is final: med2 becomes (cor, raw), NA_real_ for a cell without partners; n_cells = n_class Sq
hipError_t launch_cross_class(const double* out4, const int32_t* member, const int32_t* first, int Sr, int n_class,
                              int row_first, int n_rows, long long Sq, int stage, double* med2, int32_t* n_valid,
                              hipStream_t s);
hipError_t launch_cross_class_cor(const unsigned long long* red, int scale_max, const int32_t* n_valid, long long n_cells,
                                  double* med2, hipStream_t s);
// ---- pairs past a threshold, compacted in combn order (icikt_edges.hip) ----
struct EdgeRule {              // == icikt_edge_rule: a NaN bound is no bound
  double min_raw, max_pvalue, min_completeness;
  int absolute;
};
// the kept edges as planes of `cap` slots each: every store is a plain 4- or 8-byte one
struct EdgeOut {
  int32_t *ei, *ej;
  double *cor, *raw, *pvalue, *taumax, *completeness;
  long long cap;
};
// tiles of a block of n_pairs pairs: words of `counts` and `bases`, and a 16th of the words of `ballots`
long long edge_tiles(long long n_pairs);
constexpr int EDGE_TILE_WORDS = 16;
// out4: the records of n_pairs consecutive pairs of combn(S, 2) from pair `first` on (S <= 65 535).  The block's matching
// pairs are counted into *total (a device word the caller zeroes before a call's first block) and degree ([S], zeroed
// likewise, may be null), and those whose rank among ALL matching pairs so far is below E.cap are stored at that rank.
hipError_t launch_edge_block(const EdgeRule& R, const double* out4, long long n_pairs, long long first, int S,
                             unsigned long long* ballots, uint32_t* counts, unsigned long long* bases,
                             unsigned long long* total, unsigned long long* degree, const EdgeOut& E, hipStream_t s);
// E.cor of the first n edges (n <= E.cap); red: launch_out_stats' record
hipError_t launch_edge_finish(const EdgeOut& E, long long n, const unsigned long long* red, int scale_max, hipStream_t s);
// ---- per-sample medians within classes (icikt_medians.hip) ----
// Where a sample's partners lie in the kept plane: its class has size[s] members (ascending sample index), the sample
// is member pos[s], and the class's combn triangle starts at pair base[s] of the call's pair order.
struct MedianClasses {
  const int32_t* pos;    // [S]
  const int32_t* size;   // [S]
  const long long* base; // [S]
};
constexpr int MEDIAN_STAGE_MAX = 4096;   // keys of k_median_select's LDS staging buffer (32 KB: four workgroups per CU)
// kept[e] = the sortable key (colsort::cor_key) of pair e's raw, NA_KEY for a pair with a reason code; e < n_pairs
hipError_t launch_median_keep(const double* out4, const int32_t* reasons, long long n_pairs, unsigned long long* kept,
                              hipStream_t s);
// med2 [2][S] (cor, raw; NA_real_ without partners), n_valid [S]; red: launch_out_stats' record; stage: partners up to
// which a sample's keys are gathered into LDS once (0 .. MEDIAN_STAGE_MAX), above it every pass re-reads the plane
hipError_t launch_median_select(const MedianClasses& mc, const unsigned long long* kept, const unsigned long long* red,
                                int S, int scale_max, int stage, double* med2, int32_t* n_valid, hipStream_t s);
// ---- per-sample medians to every class (icikt_classmat.hip) ----
constexpr int CLASS_MATRIX_MAX_CLASSES = 65535;   // k_class_select's grid is (S, n_class): the second dimension's limit
// kept: the whole combn(S, 2) plane launch_median_keep writes; member [S]: the sample indices sorted stably by class;
// first [n_class + 1]: class c is member[first[c] .. first[c + 1]).  med2 [2][n_class][S] (cor, raw; NA_real_ for a
// cell without partners), n_valid [n_class][S]; red and stage as launch_median_select takes them
hipError_t launch_class_select(const int32_t* member, const int32_t* first, const unsigned long long* kept,
                               const unsigned long long* red, int S, int n_class, int scale_max, int stage, double* med2,
                               int32_t* n_valid, hipStream_t s);
// ---- maximum spanning forest / single linkage (icikt_mst.hip) ----
constexpr int MST_MAX_ROUNDS = 17;   // components with a candidate at least halve per round (S < 2^16), and one round finds nothing
// a sample's best edge out of its component: the key of its raw (0: none) and the partner (-1: none)
struct MstBest {
  unsigned long long key;
  int32_t t, pad;
};
// kept: the whole combn(S, 2) plane launch_median_keep writes; comp [S]: a component label per sample; live [S]: 0 for
// the samples of a component that found no candidate in an earlier round; min_key: colsort::cor_key of min_raw, 0 for
// no bound.  best[s]: the best candidate edge (s, t) with comp[t] != comp[s] -- the largest key that is not NA_KEY and
// not below min_key, equal keys by the smaller t
hipError_t launch_mst_best(const unsigned long long* kept, const int32_t* comp, const int32_t* live,
                           unsigned long long min_key, int S, MstBest* best, hipStream_t s);
// ---- complete, average and single linkage (icikt_hclust.hip) ----
constexpr int HCLUST_COMPLETE = 0, HCLUST_AVERAGE = 1, HCLUST_SINGLE = 2;   // == ICIKT_HCLUST_*
constexpr int HCLUST_GRID_MAX = 256;   // workgroups of the rescan kernel (hcgrid)
// the call's device state, HC_WORDS int32 words zeroed before the first scan: the call has ended; the merges recorded;
// the entries of the rescan list; the step's slots a < b and their sizes before the merge
constexpr int HC_DONE = 0, HC_MERGES = 1, HC_COUNT = 2, HC_A = 3, HC_B = 4, HC_NA = 5, HC_NB = 6, HC_WORDS = 8;
// merge record t: slot b merged into slot a < b at the similarity `key` (colsort::cor_key), the new cluster's samples
struct HcMerge {
  int32_t a, b;
  unsigned long long key;
  int32_t size, pad;
};
static_assert(sizeof(HcMerge) == 24, "a merge record is 24 bytes");
// kept: the whole combn(S, 2) plane launch_median_keep writes.  W [S][S]: the symmetric table of keys, NA_KEY on the
// diagonal; alive [S] = 1, size [S] = 1
hipError_t launch_hc_expand(const unsigned long long* kept, int S, unsigned long long* W, int32_t* alive, int32_t* size,
                            hipStream_t s);
// nn / nnkey of the rows list[0 .. state[HC_COUNT]) (all != 0: of every row, list unread): the row's best live partner --
// the largest key that is not NA_KEY, equal keys by the smaller partner -- or -1 and key 0.  grid: 1 .. HCLUST_GRID_MAX
hipError_t launch_hc_rescan(const unsigned long long* W, const int32_t* alive, const int32_t* list, const int32_t* state,
                            int S, int all, int grid, int32_t* nn, unsigned long long* nnkey, hipStream_t s);
// the step's merge: the best (nnkey[i], min(i, nn[i]), max(i, nn[i])) over live i, recorded as rec[state[HC_MERGES]];
// state[HC_DONE] = 1 when no key is left or the best is below min_key (colsort::cor_key of min_raw, 0: no bound)
hipError_t launch_hc_pick(const int32_t* nn, const unsigned long long* nnkey, int32_t* alive, int32_t* size,
                          int32_t* state, HcMerge* rec, unsigned long long min_key, int S, hipStream_t s);
// row and column a of W after the merge pick published (method: HCLUST_*), the neighbours that follow from it, and the
// rows whose neighbour was a or b -- and a -- on the list
hipError_t launch_hc_merge(unsigned long long* W, int32_t* nn, unsigned long long* nnkey, const int32_t* alive,
                           int32_t* list, int32_t* state, int method, int S, hipStream_t s);
// ---- ANOSIM: class separation under 1 - raw with its permutation test (icikt_anosim.hip) ----
constexpr int ANO_ROW_RUN = 256;          // rows of a workgroup's run
constexpr int ANO_STRIP_MIN = 1, ANO_STRIP_MAX = 4096, ANO_STRIP_DEFAULT = 256;   // columns of a workgroup's strip (anostrip)
// kept: the whole combn plane launch_median_keep writes (n keys).  *total += the keys that are not NA_KEY; dhist [8][256]
// += the keys (NA_KEY included) per digit and digit value.  The caller zeroes total and dhist.
hipError_t launch_anosim_count(const unsigned long long* kept, long long n, unsigned long long* total,
                               unsigned long long* dhist, hipStream_t s);
// sorted: the plane's keys ascending (launch_padj_sort_pass), the m values first.  r2[e] = 2 m - lo - hi + 1 with lo the
// keys below kept[e] and hi the keys at or below it: the doubled average rank in descending order; 0 for NA_KEY
hipError_t launch_anosim_rank(const unsigned long long* kept, const unsigned long long* sorted, long long n, long long m,
                              unsigned long long* r2, hipStream_t s);
// cls [S] in 0 .. n_class - 1; class_w2 / class_nw [n_class] (zeroed by the caller) += r2 / 1 per value whose two
// samples are both of the class
hipError_t launch_anosim_classes(const unsigned long long* r2, const int32_t* cls, int S, unsigned long long* class_w2,
                                 unsigned long long* class_nw, hipStream_t s);
// labT [n_groups][S][ANO_PB] halfwords: labelling g * ANO_PB + p gives sample s the class labT[(g * S + s) * ANO_PB + p].
// w2 / nw [n_groups][ANO_PB] (zeroed by the caller) += r2 / 1 per value whose two samples share a class under the
// labelling; nw only with count_nw (without an NA pair in the plane it follows from the class sizes).  strip: the
// columns of a workgroup, ANO_STRIP_MIN .. ANO_STRIP_MAX
hipError_t launch_anosim_perm(const unsigned long long* r2, const uint16_t* labT, int S, int n_groups, int strip,
                              int count_nw, unsigned long long* w2, unsigned long long* nw, hipStream_t s);
// ---- PERMANOVA: the sums of squared dissimilarities (1 - raw)^2 per class and labelling (icikt_permanova.hip) ----
// (the label plane and the batch keys are icikt_labels.h's, the strip is ANOSIM's; a run of rows is the kernel file's own, 1 024)
constexpr int PMV_T_NA = 0, PMV_T_LO = 1, PMV_T_HI = 2, PMV_TOTALS = 3;   // the words of launch_pmv_quant's totals
constexpr int PMV_LDS_CLASSES = 2048;     // classes up to which k_pmv_classes keeps a labelling's bins in LDS (16 bytes each)
// kept: the whole combn plane launch_median_keep writes (n keys).  q[e] = fixed::quantise_key(kept[e]) (icikt_fixed.h: 0
// for NA_KEY); totals[PMV_T_NA] += the NA_KEY pairs, totals[PMV_T_LO] / [PMV_T_HI] += the low 32 bits / the rest of
// every q.  The caller zeroes totals.
hipError_t launch_pmv_quant(const unsigned long long* kept, long long n, unsigned long long* q,
                            unsigned long long* totals, hipStream_t s);
// labT as launch_anosim_perm takes it.  colsum_lo / colsum_hi [n_groups][S][ANO_PB] (zeroed by the caller) += the low 32
// bits / the rest of partial sums of q over the pairs (i, j), i < j, whose samples share a class under the labelling,
// at column j's slot: sum = hi 2^32 + lo
hipError_t launch_pmv_perm(const unsigned long long* q, const uint16_t* labT, int S, int n_groups, int strip,
                           unsigned long long* colsum_lo, unsigned long long* colsum_hi, hipStream_t s);
// bins_lo / bins_hi [n_lab][n_class] (zeroed by the caller) += colsum_lo / colsum_hi of every column at the column's
// class under labelling l < n_lab; every label of labT must be below n_class
hipError_t launch_pmv_classes(const uint16_t* labT, const unsigned long long* colsum_lo,
                              const unsigned long long* colsum_hi, int S, int n_class, long long n_lab,
                              unsigned long long* bins_lo, unsigned long long* bins_hi, hipStream_t s);
// ---- Mantel: 1 - raw against another matrix of the same samples, with its permutation test (icikt_mantel.hip) ----
// (the label plane -- a permutation is a labelling with S classes -- and the batch keys are icikt_labels.h's, the strip is ANOSIM's)
constexpr int MANTEL_ROW_RUN = 1024;      // rows of a workgroup's run in k_mantel_perm
constexpr int MANTEL_M_S_LO = 0, MANTEL_M_S_HI = 1, MANTEL_M_Q_LO = 2, MANTEL_M_Q_HI = 3, MANTEL_MOMENTS = 4;   // launch_mantel_moments' words
// plane [n]: finite doubles y become the sortable keys of -y, in place
hipError_t launch_mantel_ykeys(unsigned long long* plane, long long n, hipStream_t s);
// yv[e] = mantel::quantise_y(y[e], lo, ex) (icikt_mantel.h) of the finite doubles y [n]; yv is another plane
hipError_t launch_mantel_yquant(const unsigned long long* y, long long n, double lo, int ex, unsigned long long* yv,
                                hipStream_t s);
// plane: a value below 2^32 per pair of combn(S, 2).  tab [S][S] 32-bit words: tab[i][j] = tab[j][i] = the pair's value,
// 0 on the diagonal; every cell written
hipError_t launch_mantel_expand(const unsigned long long* plane, int S, uint32_t* tab, hipStream_t s);
// kept: the whole combn plane launch_median_keep writes (n keys).  xv[e] = mantel::quantise_x of the key's double, 0 for
// NA_KEY; *n_na (zeroed by the caller) += the NA_KEY pairs
hipError_t launch_mantel_xquant(const unsigned long long* kept, long long n, unsigned long long* xv,
                                unsigned long long* n_na, hipStream_t s);
// out [MANTEL_MOMENTS] (zeroed by the caller) += the limbs of v and of v^2, v the low 32 bits of plane[e], e < n
hipError_t launch_mantel_moments(const unsigned long long* plane, long long n, unsigned long long* out, hipStream_t s);
// permT [n_groups][S][ANO_PB] halfwords as launch_anosim_perm's labT, every entry below S: permutation g * ANO_PB + p
// sends sample s to permT[(g * S + s) * ANO_PB + p].  t_lo / t_hi [n_groups][ANO_PB] (zeroed by the caller) += the low 32
// bits / the rest of xv[(i, j)] * tab[pi(i)][pi(j)] over the pairs i < j: T = hi 2^32 + lo.  strip as launch_anosim_perm
hipError_t launch_mantel_perm(const unsigned long long* xv, const uint32_t* tab, const uint16_t* permT, int S, int n_groups,
                              int strip, unsigned long long* t_lo, unsigned long long* t_hi, hipStream_t s);
// ---- PERMDISP: every sample's sum of squared dissimilarities to every class (icikt_permdisp.hip) ----
constexpr long long DISP_MAX_CELLS = 1ll << 26;   // == ICIKT_PERMDISP_MAX_CELLS: S n_class, 16 bytes a cell
// kept: the whole combn(S, 2) plane launch_median_keep writes; cls [S]: a class in 0 .. n_class - 1 per sample (checked
// by the host).  t_lo / t_hi [S][n_class] = the low 32 bits / the rest of q = fixed::quantise_key(key) summed over the
// partners t != s of class c: T = hi 2^32 + lo.  Every cell is written (above PMV_LDS_CLASSES classes the table is
// zeroed here and added to).  totals (PMV_T_*, zeroed by the caller) += the NA_KEY pairs and the limbs of every q, each
// pair once: launch_pmv_quant's totals
hipError_t launch_disp_table(const unsigned long long* kept, const int32_t* cls, int S, int n_class,
                             unsigned long long* t_lo, unsigned long long* t_hi, unsigned long long* totals,
                             hipStream_t s);
// ---- PCoA: principal coordinates of the samples under 1 - raw (icikt_pcoa.hip) ----
// Blocks of vectors are column-major with the leading dimension S: X[i + S c].  Every floating-point sum below has a
// fixed order for a given shape; the only atomic is the integer NA count of launch_pcoa_rows.
constexpr int PCOA_MAX_BLOCK = 64;        // == ICIKT_PCOA_MAX_K: columns of a block
constexpr int PCOA_MAX_BASIS = 512;       // == ICIKT_PCOA_MAX_BASIS
// kept: the whole combn(S, 2) plane launch_median_keep writes.  row_lo / row_hi [S] = the low 32 bits / the rest of
// q = fixed::quantise_key(key) summed over the partners t != s (R = hi 2^32 + lo), every cell written;
// totals[PMV_T_NA] (zeroed by the caller) += the NA_KEY pairs, each pair once
hipError_t launch_pcoa_rows(const unsigned long long* kept, int S, unsigned long long* row_lo, unsigned long long* row_hi,
                            unsigned long long* totals, hipStream_t s);
// G [S][S] = -0.5 * (((double)q 2^-50 - (mean[i] + mean[j])) + grand[0]), q = 0 on the diagonal: every cell written.
// The plane must hold no NA_KEY (it would count as q = 0)
hipError_t launch_pcoa_centre(const unsigned long long* kept, const double* mean, const double* grand, int S, double* G,
                              hipStream_t s);
// W [S x b] = G V, 1 <= b <= PCOA_MAX_BLOCK; G is read once
hipError_t launch_pcoa_apply(const double* G, const double* V, int S, int b, double* W, hipStream_t s);
// C [L x b] (C[l + ldc c]) = Q^T W for Q [S x L] and W [S x b]
hipError_t launch_pcoa_qtw(const double* Q, int L, const double* W, int S, int b, int ldc, double* C, hipStream_t s);
// Out [S x b] = A Z, or with subtract Out -= A Z, for A [S x L] and Z [L x b] (Z[l + ldz c]); l ascending
hipError_t launch_pcoa_axz(const double* A, int L, const double* Z, int ldz, int S, int b, int subtract, double* Out,
                           hipStream_t s);
// out[c] = the sum of squares of X[0 .. n) + ld c, c < cols; out[0] = the sum of x [n]
hipError_t launch_pcoa_sumsq(const double* X, int n, long long ld, int cols, double* out, hipStream_t s);
hipError_t launch_pcoa_sum(const double* x, int n, double* out, hipStream_t s);
// x [n] /= sqrt(sumsq[0]) and flag[0] = 1; with sumsq[0] below thr2 (or 0) x = 0 and flag[0] = 0
hipError_t launch_pcoa_scale(double* x, int n, const double* sumsq, double thr2, int32_t* flag, hipStream_t s);
// out[c] = |GY_c - theta[c] Y_c|^2, c < k
hipError_t launch_pcoa_resid(const double* GY, const double* Y, const double* theta, int S, int k, double* out,
                             hipStream_t s);
// every column of Y [S x k]: negated iff its component of largest magnitude (the smallest index among equals) is negative
hipError_t launch_pcoa_sign(double* Y, int S, int k, hipStream_t s);
// ---- quantiles and histogram of all pairs (icikt_quantiles.hip) ----
constexpr int QUANT_MAX_BINS = 1024;    // == ICIKT_HIST_MAX_BINS: k_quant_fold stages 1 025 breaks and 2 x 1 026 counters in LDS
constexpr int QUANT_HEAD = 4;           // words of a counted group before its bins: n_valid, n_na, below, above
constexpr int QUANT_BATCH_MAX = 32;     // targets of one select batch: k_quant_count holds 32 x 256 counters (32 KB) in LDS
// the select's targets: the key of rank `rank` (0-based, among the valid keys ascending) of group `group` (0 every
// pair, 1 cls[i] == cls[j], 2 the others); prefix starts at 0 and is the key after the eighth pass
struct QuantTargets {
  unsigned long long* prefix;
  long long* rank;
  int32_t* group;
};
// out4 / reasons: the records of n_pairs consecutive pairs of combn(S, 2) from pair `first` on (S <= 65 535).  totals:
// per counted group c (0 every pair; 1 cls[i] == cls[j], only with cls) QUANT_HEAD + max(n_breaks - 1, 0) words from
// c times that on, added to (the caller zeroes them before a call's first block): n_valid, n_na, raw below breaks[0],
// raw above the last break, then the bins as numpy.histogram counts them.  breaks: n_breaks (0, or 2 ..
// QUANT_MAX_BINS + 1) device doubles, strictly increasing.  kept (may be null): the whole plane, one sortable key
// (colsort::cor_key, NA_KEY for a pair with a reason code) per pair of the triangle, written at first + e.
hipError_t launch_quant_fold(const double* out4, const int32_t* reasons, long long n_pairs, long long first, int S,
                             const int32_t* cls, const double* breaks, int n_breaks, unsigned long long* kept,
                             unsigned long long* totals, hipStream_t s);
// one digit (shift = 56, 48 .. 0, in this order) of the radix select over the kept plane of all n_pairs pairs for
// targets [t0, t0 + nt), nt <= QUANT_BATCH_MAX: count adds to hist [nt][256] (zeroed before the first pass), pick
// extends the targets' prefixes, reduces their ranks and zeroes hist again
hipError_t launch_quant_count(const unsigned long long* kept, long long n_pairs, int S, const int32_t* cls,
                              const QuantTargets& T, int t0, int nt, int shift, unsigned long long* hist, hipStream_t s);
hipError_t launch_quant_pick(const QuantTargets& T, int t0, int nt, int shift, unsigned long long* hist, hipStream_t s);
// ---- multiple-testing adjustment of all pairs (icikt_padjust.hip) ----
constexpr int PADJ_BONFERRONI = 0, PADJ_HOLM = 1, PADJ_HOCHBERG = 2, PADJ_BH = 3;   // == ICIKT_ADJUST_*
constexpr int PADJ_MAX_ALPHA = 16;              // == ICIKT_ADJUST_MAX_ALPHA
constexpr long long PADJ_MAX_TILES = 65536;     // tiles of a sort pass: 256 counters of 8 bytes each per tile (128 MB)
constexpr int PADJ_SCAN_CHUNK = 1024;           // items a workgroup of a chip-wide scan reduces and scans at a time
constexpr int PADJ_CUT_WORDS = 2 * PADJ_MAX_ALPHA + 1;   // launch_padj_cut's record
// the keys a wave's tile of the sort holds for a plane of n keys: `want` (the padjtile plan key; 0: the library's 1 024)
// raised until the plane has at most PADJ_MAX_TILES tiles
long long padj_tile(long long n, long long want);
// words of the aggregates a scan of this call needs at most (over the 256 counters of every tile, or over the n keys)
long long padj_scan_chunks(long long n, long long tile);
// out4 / reasons: the records of n_pairs consecutive pairs of combn(S, 2) from pair `first` on.  kept[first + e] = the
// pair's p-value as a sortable key (colsort::cor_key), NA_KEY for a pair with a reason code or a NaN p; *total += the
// valid keys; dhist [8][256] += the keys (NA_KEY included) per digit and digit value.  The caller zeroes total and dhist
// before a call's first block.
hipError_t launch_padj_fold(const double* out4, const int32_t* reasons, long long n_pairs, long long first, int S,
                            unsigned long long* kept, unsigned long long* total, unsigned long long* dhist,
                            hipStream_t s);
// one digit (shift = 0, 8 .. 56, in this order) of the stable radix sort of the n keys of src into dst; counts: 256 words
// per tile, agg: padj_scan_chunks words
hipError_t launch_padj_sort_pass(const unsigned long long* src, unsigned long long* dst, long long n, long long tile,
                                 int shift, unsigned long long* counts, unsigned long long* agg, hipStream_t s);
// adj[i], i < m: the adjusted value (PADJ_* method) of the i-th of the m sorted keys; agg: padj_scan_chunks words
hipError_t launch_padj_adjust(const unsigned long long* keys, long long m, int method, double* adj, double* agg,
                              hipStream_t s);
// cut [PADJ_CUT_WORDS]: per alpha (device doubles) the adjusted values <= alpha, from word PADJ_MAX_ALPHA on per alpha
// the bits of the largest p among them (NA_real_: none), in the last word the largest of the counts
hipError_t launch_padj_cut(const double* adj, const unsigned long long* keys, long long m, const double* alpha,
                           int n_alpha, unsigned long long* cut, hipStream_t s);
// the distinct keys among the first min(*extent, m) sorted positions, ascending: table [2][cap] gets the first cap of
// them as p-values and their adjusted values, *n_table their full count; agg: padj_scan_chunks words
hipError_t launch_padj_table(const unsigned long long* keys, const double* adj, long long m,
                             const unsigned long long* extent, long long cap, double* table, unsigned long long* agg,
                             unsigned long long* n_table, hipStream_t s);
// wide columns: one wave per pair, grid of `blocks` single-wave workgroups that fetch pairs from *task_ctr
hipError_t launch_k1_wide(const PrepView& pv, const int32_t* pi, const int32_t* pj, PairRaw* raw, int64_t n_pairs,
                          int blocks, size_t lds_bytes, int* task_ctr, hipStream_t s);
hipError_t k1_wide_blocks_per_cu(size_t lds_bytes, int* out);
inline size_t k1_wide_lds_bytes(int Wp) { return (size_t)(Wp + 1) * (8 + 8 + 4 + 4); }
hipError_t launch_k0_expand(const PrepView& pv, int col_begin, int ncols, hipStream_t s);
// task_ctr: nullptr = the grid covers the task list; else 8 zeroed counters, the waves fetch their tasks (whole-wave kernels)
hipError_t launch_zero_raw(const int32_t* tasks, int n_tasks, PairRaw* raw, hipStream_t s);
hipError_t launch_k1(const PrepView& pv, const int32_t* tasks, int n_tasks, const int32_t* pi,
                     const int32_t* pj, PairRaw* raw, int np, int half_items, int wpb, int blocks,
                     size_t lds_bytes, int perpair_bytes, int* task_ctr, int opts, hipStream_t s);
hipError_t k1_blocks_per_cu(int np, int half_items, int wpb, size_t lds_bytes, int* out);
hipError_t launch_k2(const PrepView& pv, const int32_t* pi, const int32_t* pj, const PairRaw* raw,
                     int64_t n_pairs, int perspective, int alternative, int continuity, int exact64,
                     double* out4, int64_t* counts, int32_t* reasons, hipStream_t s);
// the mask-only pre-pass of pairwise_completeness: missing-row bitsets (NaN = missing) of columns [col_begin, col_begin + ncols)
hipError_t launch_k0_mask(const PrepView& pv, const double* dX, int64_t ld, int col_begin, int ncols, hipStream_t s);
hipError_t launch_missingness(const PrepView& pv, const int32_t* pi, const int32_t* pj, int64_t n_pairs,
                              int64_t* missing, hipStream_t s);
hipError_t launch_mask_pairs(const double* dX, int64_t ld, int n, const int32_t* pi, const int32_t* pj, int64_t first,
                             int64_t npairs, double* dXp, hipStream_t s);
// pi / pj of pairs [begin, begin + count) of combn(S, 2) order, computed on the device
hipError_t launch_fill_combn(int32_t* pi, int32_t* pj, int64_t S, int64_t begin, int64_t count, hipStream_t s);
// ---- cor_fast (icikt_cor.hip) ----
constexpr uint32_t COR_CONSTANT = 1u;   // per side of a pair (second side << 8): no variance among the rows used
constexpr uint32_t COR_TIES = 2u;       // ... Spearman: tied ranks among them
constexpr int COR_OK = 0, COR_SHORT = 1, COR_NA = 2, COR_TIES_WARN = 3;   // == ICIKT_COR_* of include/icikt.h
// per pair: the rows used and the centred cross / square sums (Spearman: of doubled ranks, exact integers)
struct CorAcc {
  double m, sxy, sxx, syy;
  uint32_t flags, pad;
};
struct CorPrep {
  const double* X;   // the matrix on the device, NaN = NA
  int64_t ld, n;     // leading dimension, rows
  int S;             // columns
  int method;        // 0 Pearson, 1 Spearman
  double* Z;         // n x S: centred values (Pearson) / centred doubled ranks (Spearman); NA = NaN
  int32_t* cnt;      // non-NA rows per column
  double* colss;     // Pearson: Σz² - (Σz)² / n of a column's Z; Spearman: Σz²
  double* colsum;    // Σz (Spearman: 0)
  uint8_t* flags;    // COR_CONSTANT | COR_TIES per column
  int32_t *ord, *gs, *ge;   // Spearman, n x S: sorted order of the non-NA rows, each position's tie group [gs, ge)
  uint64_t* keys;    // Spearman: sort scratch, np2 per workgroup
  int32_t* idx;
  int np2;
};
hipError_t launch_cor_prep(const CorPrep& cp, int blocks, hipStream_t s);
// all pairs of combn(S, 2) order (then the S self pairs when diag) of a matrix without NA
hipError_t launch_cor_tile(const CorPrep& cp, int diag, CorAcc* acc, hipStream_t s);
hipError_t launch_cor_dots(const CorPrep& cp, int pairwise, const int32_t* pi, const int32_t* pj, int64_t P, CorAcc* acc,
                           hipStream_t s);
// scratch: blocks x (2 n + 1) int32
hipError_t launch_cor_spearman_pw(const CorPrep& cp, const int32_t* pi, const int32_t* pj, int64_t P, int blocks,
                                  int32_t* scratch, CorAcc* acc, hipStream_t s);
// prho_upper: the exact upper-tail permutation counts of Spearman's S for n = 2 .. 9 (cor_prho_table)
hipError_t launch_cor_epilogue(const CorAcc* acc, int64_t P, int method, int pairwise, int alternative, int continuity,
                               const uint32_t* prho_upper, double* out3, int32_t* reasons, hipStream_t s);
// ---- missing-value diagnostics (icikt_diag.hip) ----
// per-column pass: the rule, counts, sort, median; rank mode (rank2 != nullptr) the doubled ranks
struct DiagCol {
  const double* X;   // the matrix on the device
  int64_t ld, n;     // leading dimension, rows
  int S;             // columns
  MaskSpec ms;       // global_na rule (a NaN is missing whatever it holds)
  int na_rm;         // 0: a column with a missing cell has median NA
  double* median;    // [S] median of the non-missing values, NA_real_ / R_NaN as R's median gives
  int32_t* nmiss;    // [S] missing cells (NaN or excluded)
  int32_t* nexcl;    // [S] cells the rule excludes
  const uint8_t* kept;   // rank mode: [n] row kept (not missing in every column)
  int32_t* rank2;    // rank mode: n x S doubled rank(x, na.last = FALSE) over the kept rows (dropped rows: 0); else nullptr
  uint64_t* keys;    // sort scratch, np2 per workgroup
  int32_t *idx, *gs;
  int np2;
};
hipError_t launch_diag_col(const DiagCol& dc, int blocks, hipStream_t s);
// out3[3 k ..]: trials, successes, missing cells of class k (zeroed by the caller)
hipError_t launch_diag_censor(const double* X, int64_t ld, int64_t n, const MaskSpec& ms, const int32_t* cols,
                              const int32_t* off, int n_class, const double* median, unsigned long long* out3,
                              hipStream_t s);
hipError_t launch_diag_rowmiss(const double* X, int64_t n, int n_cols, const MaskSpec& ms, int32_t* n_na,
                               uint8_t* kept, unsigned long long* n_kept, hipStream_t s);
hipError_t launch_diag_median_rank(const int32_t* rank2, int64_t n, int n_cols, const uint8_t* kept, double* med,
                                   hipStream_t s);
hipError_t launch_diag_gather(const double* X, int64_t n, const MaskSpec& ms, const int32_t* rows, int64_t n_out,
                              const int32_t* colsel, int n_cols, double* out, hipStream_t s);
// icikt_ingest.hip: nc columns of the column-major float64 matrix dst (leading dimension dst_ld) from a device block of
// ICIKT_DTYPE_* cells in ICIKT_ORDER_* layout with leading dimension src_ld (elements)
hipError_t launch_ingest(const void* src, int dtype, int order, int64_t src_ld, int64_t n, int64_t nc, double* dst,
                         int64_t dst_ld, hipStream_t s);
// icikt_sparse.hip: nc columns of the column-major float64 matrix dst from a device block of a CSC matrix's values
// (ICIKT_DTYPE_*) and row indices (ICIKT_INDEX_*): entry e of the matrix lies at vals[e - base] / idx[e - base], the block
// holds block_nnz entries, column j's entries are [indptr[col0 + j], indptr[col0 + j + 1]) (indptr on the device); cells
// without an entry get `fill`.  An entry that is rejected is never stored through; the first rejection of a launch goes
// to err[0 .. 4): kind (ICIKT_CSC_*; 0 = none, the host clears it), column, position of the entry, row index.
enum : unsigned long long { ICIKT_CSC_BAD_ROW = 1, ICIKT_CSC_DUPLICATE = 2, ICIKT_CSC_BAD_INDPTR = 3 };
constexpr int ICIKT_CSC_ERR_WORDS = 4;
hipError_t launch_scatter_csc(const void* vals, int dtype, const void* idx, const void* indptr, int index_type,
                              int64_t col0, int64_t base, int64_t block_nnz, double fill, int64_t n, int64_t nc,
                              double* dst, int64_t dst_ld, unsigned long long* err, hipStream_t s);
hipError_t launch_selftest(uint32_t* d_out, hipStream_t s);
hipError_t read_step_stats(unsigned long long* out24, int reset);

}  // namespace icikt
#endif
