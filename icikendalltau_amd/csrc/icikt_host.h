// icikt_host.h -- host-side internals shared by the entry files of one device (icikt_capi.cpp: the pair engine's
// entries, icikt_pipeline.cpp: its copies, pre-pass and pair launches, icikt_capi_cor.cpp: cor_fast,
// icikt_capi_diag.cpp: the missing-value diagnostics) and icikt_multi.cpp (several devices, RCCL).  Internal; the
// public boundary is include/icikt.h.
#ifndef ICIKT_HOST_H
#define ICIKT_HOST_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <functional>
#include <utility>
#include <vector>

#include "icikt.h"
#include "icikt_blocks.h"
#include "icikt_device.h"
#include "icikt_k0plan.h"
#include "icikt_k1plan.h"
#include "icikt_keys.h"
#include "icikt_transfer.h"

// a device buffer, grown on demand and kept; freed with its owner (on the device current at that time)
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 64;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

struct icikt_ctx {
  int device = -1;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  hipDeviceProp_t prop{};

  // prepared matrix
  bool prepared = false;
  icikt::PrepView pv{};
  DevBuf<uint16_t> order, hirow, girow, srow;
  DevBuf<uint32_t> wide32;                 // wide columns: order32 | q32 | lo32 | hi32, S x n_pad each
  DevBuf<uint32_t> order_w;                // columns of more than 30 656 rows: `order` as 32-bit words (PrepView::order_w)
  DevBuf<unsigned long long> k0_bits;      // wide columns: K0's phase-3 bitsets, per column of a sort chunk
  DevBuf<uint32_t> rec, tgroups, tprog;
  DevBuf<uint2> smask;
  DevBuf<unsigned long long> meta, sort_keys;
  DevBuf<uint32_t> sort_idx;
  int sort_chunk = 0;
  int64_t alloc_cols = 0;  // columns the prepared-state arrays are allocated for (>= n_samp)

  // pair list
  int64_t n_pairs = -1;
  int64_t pairs_nsamp = -1;  // largest column index + 1 seen in the list
  int n_units = 0;
  int wpb = 0;  // pairs per wave (np) the tasks were built for; 0 = not built
  int group_hint = 0;      // ... and the size of the tie group a random tied pair of their rows sits in (fill groups apart)
  int ntg_hint = -1;       // the most tie groups among the columns whose statistics matrix_tied() read back (-1: not read)
  int tied_state = -1;     // 15 200 .. 30 656 rows (and longer columns: pairs per wave): do the prepared columns hold many tie groups (1), not (0), not asked yet (-1)
  bool raw_valid = false;  // d_raw holds the pair kernel's counts for the current prepared matrix and pair list
  DevBuf<int32_t> d_pi, d_pj, d_unit_start;
  DevBuf<icikt::PairRaw> d_raw;
  DevBuf<int> d_task_ctr;  // persistent pair kernel: one task counter per XCD group, zeroed before every launch
  std::vector<int32_t> h_pi, h_pj, h_units;
  // a combn range [combn_begin, combn_end) of combn(combn_S, 2) set by icikt_set_pairs_combn: the device arrays are
  // filled by a kernel at once, the host copies (h_pi / h_pj: only the host-built task lists read them) on demand
  int64_t combn_S = -1, combn_begin = 0, combn_end = 0;
  bool h_pairs_valid = false;
  bool units_dirty = false;   // h_units has been rebuilt on the host and not uploaded yet
  icikt::host::Transfers xfer;   // the pinned buffers, threads and events that move caller memory (icikt_transfer.h)

  // host-path staging: a second stream for H2D copies that run ahead of K0 by column chunks
  hipStream_t copy_stream = nullptr;
  // the pipelined host path (icikt_pairs_f64 / icikt_matrix_f64 on a matrix of several chunks): the pre-pass of chunk
  // k runs on its own stream as soon as the chunk has arrived, and the pair kernel -- one launch per chunk, over the
  // tasks whose LAST column lies in it -- follows on the context's stream while later chunks still cross PCIe
  hipStream_t prep_stream = nullptr;
  std::vector<hipEvent_t> ev_chunk;        // pre-pass of chunk k done
  std::vector<int64_t> chunk_col_end;      // columns [.., chunk_col_end[k]) have arrived with chunk k (this call)
  int pipe_mode = -1;                      // -1: the library's choice; 0 / 1: off / on whenever possible (debug plan)
  DevBuf<double> d_X, d_out4, d_Xp;  // d_Xp: masked column pairs of icikt_pairs_complete_f64
  DevBuf<unsigned char> d_ingest;    // chunks of a view that is not column-major float64, as uploaded (two halves: MatrixUpload)
  DevBuf<unsigned char> d_indptr;    // a CSC view's column offsets, uploaded once per call
  DevBuf<unsigned long long> d_csc_err;   // k_scatter_csc's error record (ICIKT_CSC_ERR_WORDS words)
  // full-matrix entry (icikt_matrix_f64): the exclusion rule the pre-pass applies while it reads the matrix and the
  // optional keep bytes it writes (both only for the duration of that call), the assembled matrices, the reduction
  DevBuf<double> d_out5;
  DevBuf<uint8_t> d_keep;
  DevBuf<unsigned long long> d_red;
  DevBuf<int32_t> d_pi_all, d_pj_all;     // icikt_matrix_multi_f64, explicit pair list: the whole list on the first device
  bool k0_small = false;    // (no caller sets it: the 256-thread shape of the pre-pass is reached through the plan key only)
  int k0_shape = -1;        // debug plan key "k0": -1 the library's choice (icikt_k0plan.h), 0 the large shape, 1 the small one, 2 the 512-thread one
  const icikt::MaskSpec* k0_mask = nullptr;
  uint8_t* k0_keep = nullptr;
  DevBuf<int64_t> d_counts;
  DevBuf<int32_t> d_reasons;
  DevBuf<uint32_t> d_self;

  // cor_fast (icikt_cor_pairs_f64)
  struct CorBufs {
    DevBuf<double> z, colss, colsum;
    DevBuf<int32_t> cnt, order, scratch;   // order: ord | gs | ge, n x S each
    DevBuf<uint8_t> flags;
    DevBuf<unsigned long long> keys;
    DevBuf<icikt::CorAcc> acc;
    DevBuf<uint32_t> prho;                  // exact upper tails of Spearman's S, n = 2 .. 9 (uploaded once)
    bool prho_ready = false;
  } cor;

  // top-k partners per sample (icikt_topk_f64): the columns' lists (TopkLists), their state words and the results
  struct TopkBufs {
    DevBuf<unsigned long long> key;
    DevBuf<int32_t> partner, state, idx, n_valid;
    DevBuf<double> vals, out;
  } topk;

  // query x reference rectangle (icikt_cross_f64): the five planes [5][Sq Sr] when the matrices are asked for, and the
  // queries' lists (idx [Sq][k], out [5][Sq][k], n_valid [Sq]); with class labels on the reference (icikt_ref_cross_f64)
  // the reference columns sorted by class with each class's range, and the results per (class, query) cell
  struct CrossBufs {
    DevBuf<double> planes, out, med2;
    DevBuf<int32_t> idx, n_valid, member, first, cls_n_valid;
  } cross;

  // a reference that stays prepared (icikt_ref_prepare_f64): device columns [0, n_reference) of d_X and of the prepared
  // state hold the reference, pre-passed under `ms`; the query batches of icikt_ref_cross_f64 land at
  // ref_query_col(n_reference).  Dropped (valid = false) by whatever replaces the prepared state: prepare_alloc,
  // mask_alloc, forget_prepared.
  struct RefState {
    bool valid = false;
    int64_t n_feat = 0, n_reference = 0, capacity = 0;
    icikt::MaskSpec ms{};
  } ref;

  // pairs past a threshold (icikt_edges_f64): a block's ballot words, tile counts and tile bases, the running total
  // (word 0 of `total`), the degrees and the planes of the kept edges
  struct EdgeBufs {
    DevBuf<unsigned long long> ballots, bases, total, degree;
    DevBuf<uint32_t> counts;
    DevBuf<int32_t> ei, ej;
    DevBuf<double> vals;   // [5][cap]: cor, raw, pvalue, taumax, completeness
  } edges;

  // the key planes and the sort's scratch of the selection entries, one set for all of them (DESIGN.md section 16 says
  // who leaves what there): `kept` is the call's plane, one sortable key per pair of the call; plane_a and plane_b are
  // what a sort ping-pongs between and what takes a rank or adjust pass afterwards (select_sort); counts are the
  // sort's (digit, tile) counters, agg a scan's chunk aggregates, total and dhist the valid count and the digit table
  // of the fold that feeds the sort
  struct SelectWork {
    DevBuf<unsigned long long> kept, plane_a, plane_b, counts, agg, total, dhist;
  } sel;
  // the label plane of the permutation-test entries: one batch of labellings as halfwords (select_labellings)
  DevBuf<uint16_t> labels;

  // per-sample medians within classes (icikt_class_medians_f64): the samples' places in their classes (MedianClasses)
  // and the results; the computed pairs' keys are in sel.kept
  struct MedianBufs {
    DevBuf<int32_t> pos, size, n_valid;
    DevBuf<long long> base;
    DevBuf<double> med2;
  } med;

  // per-sample medians to every class (icikt_class_matrix_f64): the samples sorted by class with each class's range,
  // and the results per (class, sample) cell; the triangle's keys are in sel.kept
  struct ClassMatBufs {
    DevBuf<int32_t> member, first, n_valid;
    DevBuf<double> med2;
  } cmat;

  // quantiles and histogram of all pairs (icikt_quantiles_f64): the class index, the breaks, the counted groups' totals,
  // and the select's targets (QuantTargets) with their digit histograms; the triangle's keys are in sel.kept, only when
  // quantiles are asked for
  struct QuantBufs {
    DevBuf<unsigned long long> totals, prefix, hist;
    DevBuf<long long> rank;
    DevBuf<int32_t> group, cls;
    DevBuf<double> breaks;
  } quant;

  // multiple-testing adjustment of all pairs (icikt_padjust_f64): the alphas, the cut-offs' record, the table's count
  // and the table itself; the keys, the sort and the adjusted values are in sel (kept, plane_a)
  struct PadjBufs {
    DevBuf<unsigned long long> cut, n_table;
    DevBuf<double> alpha, table;
  } padj;

  // maximum spanning forest (icikt_mst_f64): the samples' component labels and live flags, and every sample's best
  // edge of a round; the triangle's keys are in sel.kept
  struct MstBufs {
    DevBuf<int32_t> comp, live;
    DevBuf<icikt::MstBest> best;
  } mst;

  // complete, average and single linkage (icikt_hclust_f64): the symmetric S x S table of keys, every slot's cached
  // neighbour with its key, the live flags and cluster sizes, the rescan list, the call's state words (icikt_device.h:
  // HC_*) and the merge records; the triangle's keys are in sel.kept
  struct HclustBufs {
    DevBuf<unsigned long long> table, nnkey;
    DevBuf<int32_t> nn, alive, size, list, state;
    DevBuf<icikt::HcMerge> rec;
  } hc;

  // ANOSIM (icikt_anosim_f64): the observed labelling and its per-class sums, and the sums of a batch of labellings
  // (the batch itself: labels); the keys, their sorted copy and the doubled ranks are in sel (kept, plane_a, plane_b)
  struct AnosimBufs {
    DevBuf<unsigned long long> class_sums, w2, nw;
    DevBuf<int32_t> cls;
  } ano;

  // PERMANOVA (icikt_permanova_f64): the two limbs of the columns' sums and of the bins of a batch of labellings (the
  // batch itself: labels), and the call's totals (NA pairs, Q's limbs); the keys and their fixed-point values are in
  // sel (kept, plane_a)
  struct PermanovaBufs {
    DevBuf<unsigned long long> colsum_lo, colsum_hi, bins_lo, bins_hi, totals;
  } pmv;

  // Mantel (icikt_mantel_f64): the symmetric S x S table of the other matrix's integers, the two limbs of T of a batch of
  // permutations (the batch itself: labels), and the call's words (x's moments, y's moments, the NA pairs); `other`, its
  // keys and ranks pass through sel (kept, plane_a, plane_b) before the first block, x's keys and integers after it
  struct MantelBufs {
    DevBuf<uint32_t> table;
    DevBuf<unsigned long long> t_lo, t_hi, words;
  } mantel;

  // PERMDISP (icikt_permdisp_f64): the class of every sample, the two limbs of the S x n_class table and the call's
  // totals (NA pairs, Q's limbs); the keys are in sel.kept
  struct PermdispBufs {
    DevBuf<unsigned long long> t_lo, t_hi, totals;
    DevBuf<int32_t> cls;
  } disp;

  // PCoA (icikt_pcoa_f64): the two limbs of the row sums and the NA count, the means, the centred S x S table, the
  // Krylov basis with its image under the table (S x max_basis each), a block's scratch, the Ritz vectors with their
  // image, and the small buffers (coefficients, Ritz coefficients and values, norms, flags); the keys are in sel.kept
  struct PcoaBufs {
    DevBuf<unsigned long long> row_lo, row_hi, totals;
    DevBuf<double> mean, table, basis, image, block, y, gy, coef, z, small;
    DevBuf<int32_t> flags;
  } pcoa;

  // missing-value diagnostics (icikt_col_medians_f64, icikt_censor_counts_f64, icikt_rank_order_f64)
  struct DiagBufs {
    DevBuf<double> median, medrank, out;
    DevBuf<int32_t> nmiss, nexcl, nna, rank2, idx, gs, lists;   // lists: the host-built row / column index lists
    DevBuf<uint8_t> kept;
    DevBuf<unsigned long long> keys, red;
  } diag;

  // launch-plan overrides of the pair kernel (icikt_debug_set_plan; icikt_k1plan.h)
  using PlanOverride = icikt::host::PlanOverride;
  PlanOverride plan_ov;

  // timing
  // per kernel id a pool of HIP event pairs: several timed launches per step accumulate without a host stall
  // and are folded into ms[] when the figures are read (or when the pool is full)
  struct EvPair { hipEvent_t a = nullptr, b = nullptr; };
  std::vector<EvPair> ev_pool[ICIKT_K_COUNT];
  size_t ev_used[ICIKT_K_COUNT] = {};
  bool ev_open[ICIKT_K_COUNT] = {};
  double ms[ICIKT_K_COUNT] = {};
  int64_t launches[ICIKT_K_COUNT] = {};
};


namespace icikt {
namespace host {

int fail(icikt_ctx* c, int code, const std::string& msg);
int use_device(icikt_ctx* c);
// entry checks and timers shared by the entry files (defined in icikt_capi.cpp)
// matrix shape of an entry, `who` prefixing the message; wide_ok: the entry has a path for columns past ICIKT_MAX_FEATURES
int check_shape(icikt_ctx* c, const char* who, int64_t n_feat, int64_t n_samp, int64_t ld, bool wide_ok = true);
// the matrix of a host entry as a view: the view itself (null, dtype, order), check_shape with the view's leading
// dimension (COL: ld >= n_feat; ROW: ld >= n_samp), and null data for a matrix with cells
int check_view(icikt_ctx* c, const char* who, const icikt_input* X, int64_t n_feat, int64_t n_samp, bool wide_ok = true);
// the matrix of a host entry as a dense view or a CSC view (MatrixSrc): check_view, or for a CSC view the view itself
// (null, dtype, index_type), check_shape, indptr (null, indptr[0] < 0, decreasing: O(n_samp)) and null values / indices
// for a matrix with entries
int check_src(icikt_ctx* c, const char* who, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, bool wide_ok = true);
// every index of a host pair list inside [0, n_samp)
int check_pair_list(icikt_ctx* c, const char* who, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int64_t n_samp);
// with ICIKT_FLAG_TIMING: an event pair of kernel id k (ICIKT_K_*) around what the caller puts on c->stream in between
int timer_begin(icikt_ctx* c, int k, uint32_t flags);
int timer_end(icikt_ctx* c, int k, uint32_t flags);

#define HIPCHK(c, call)                                                                               \
  do {                                                                                                \
    hipError_t e__ = (call);                                                                          \
    if (e__ != hipSuccess)                                                                            \
      return icikt::host::fail((c), ICIKT_E_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// The end of a call that left its own scratch columns and pair list in the context, nothing of the caller's (the
// selection entries, icikt_pairs_complete_*): forget the prepared state and the pair list.  The device-resident calls
// start over (icikt_run_dev: ICIKT_E_STATE until icikt_prepare_dev and a pair list; icikt_num_pairs: -1), and a
// prepared reference is gone (icikt_ref_cross_*: ICIKT_E_STATE).
inline void forget_prepared(icikt_ctx* c) {
  c->ref.valid = false;   // (icikt_ref_cross_* alone puts it back: its blocks run beside the reference's tables)
  c->prepared = false;
  c->raw_valid = false;
  c->n_pairs = -1;
  c->pairs_nsamp = -1;
  c->wpb = 0;
  c->combn_S = -1;
}

// ---- what enqueues copies, the pre-pass and the pair launches (icikt_pipeline.cpp) ----
// Allocate the prepared state of an n_feat x n_samp matrix for alloc_cols >= n_samp columns (sort scratch for
// sort_cols columns at a time) and set c->pv.  No kernel is launched.
int prepare_alloc(icikt_ctx* c, int64_t n_feat, int64_t n_samp, int64_t alloc_cols, int64_t sort_cols);
// K0 over columns [col_begin, col_end) of the device matrix dX (leading dimension ld) on c->stream.
int prepare_launch(icikt_ctx* c, const double* dX, int64_t ld, int64_t col_begin, int64_t col_end, hipStream_t stream = nullptr);
// Host matrix -> device (columns [col_begin, col_end) only) overlapped with K0 by column chunks; the device copy
// keeps the full n_feat x n_samp layout (leading dimension n_feat) in c->d_X.  prepare_alloc() must have run.
// pipelined: the pre-pass launches go to c->prep_stream, one event per chunk in c->ev_chunk / c->chunk_col_end; the
// caller makes c->stream wait for them (per chunk, or for the last one), and synchronises c->copy_stream before it
// returns to ITS caller.  prepass: what runs over a chunk once it has arrived (kPrepass*, icikt_k0plan.h, which also
// says how many columns a chunk holds).
// Allocate c->pv for the missing-row bitsets alone (meta; no order / rec / sort scratch).  Leaves the context unprepared.
int mask_alloc(icikt_ctx* c, int64_t n_feat, int64_t n_samp);
int upload_and_prepare(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, int64_t col_begin,
                       int64_t col_end, uint32_t flags, bool pipelined = false,
                       const std::function<int(size_t, int64_t)>* on_chunk = nullptr,   // pipelined: called per chunk (index, columns arrived)
                       int prepass = kPrepassFull);
// H2D + pre-pass + pair kernel of the host entries: pipelined by chunks when the matrix has several, else in sequence.
// Leaves the pair kernel's counts in c->d_raw (raw_valid): the caller runs the epilogue (icikt_run_dev with
// ICIKT_FLAG_REUSE_COUNTS).
int upload_prepare_pairs(icikt_ctx* c, const MatrixSrc& X, int64_t n_feat, int64_t n_samp, uint32_t flags);
// The tie verdict (matrix_tied) on the first min(64, pv.n_samp) prepared columns now, where a plan asks for one: it is
// kept until the next prepare_launch.  Waits for c->stream when it reads the statistics back.
void settle_tie_verdict(icikt_ctx* c);
// global_na values (NaN = NA, +-Inf = Inf, anything else compared with ==) -> the pre-pass's exclusion rule
int make_mask_spec(icikt_ctx* c, const double* global_na, int n_global_na, icikt::MaskSpec* ms);
// Build the pair kernel's task list on the host now (prepare_alloc and a pair list must be in place).
void prebuild_units(icikt_ctx* c);
// The context's host pair list (h_pi / h_pj, n_pairs) onto the device; reserves d_raw for it.
int upload_pairs(icikt_ctx* c);
// The counts step of icikt_run_dev: the pair kernel -- the wide one, or the plan's over the whole task list (rebuilt and
// uploaded when the plan or the pair list changed) -- over the prepared matrix and the pair list, inside an
// ICIKT_K_PAIRS timer pair; leaves the counts in c->d_raw (raw_valid).
int run_counts(icikt_ctx* c, uint32_t flags);
// The arguments the pair and matrix entries share, `who` prefixing the message: shape, null matrix, pair list (none: all
// pairs, *n_pairs set), null output (out5: needed for any column, out4: for any pair), perspective and alternative.
int check_pair_args(icikt_ctx* c, const char* who, const MatrixSrc& X, int64_t n_feat, int64_t n_samp,
                    const int32_t* pi, const int32_t* pj, int64_t* n_pairs, const void* out, bool out5,
                    int perspective, int alternative);

// ---- the selection entries (icikt_topk_*, icikt_edges_*, icikt_class_medians_*, icikt_quantiles_*, icikt_class_matrix_*, icikt_padjust_*, icikt_mst_*, icikt_anosim_*, icikt_hclust_*, icikt_permanova_*, icikt_permdisp_*) and icikt_cross_*: one driver, icikt_capi_select.cpp ----
// (the blocks a call runs in: icikt_blocks.h; DESIGN.md "adding a selection entry")
// the arguments the entries share
struct SelectArgs {
  const double* global_na;
  int n_global_na;
  int perspective, alternative, continuity;
  uint32_t flags;
  double* max_taumax;
  int64_t* reason_counts;
};
// one call of an entry: `who` prefixes its messages; ms is the exclusion rule select_check_args makes of global_na
struct SelectCall {
  icikt_ctx* c;
  const char* who;
  const MatrixSrc& X;
  int64_t n_feat, n_samp;
  SelectArgs A;
  icikt::MaskSpec ms;
};
// what an entry adds to the driver's call sequence, all on c->stream
struct SelectSteps {
  std::function<int()> upload;                        // (optional) the entry brings the device matrix and its pre-pass itself -- icikt_cross_*:
                                                      // two sources -- in place of the driver's upload of s.X; the blocks then run one after the other
  std::function<int()> start;                         // its own device state, before the first block
  std::function<int(const PairBlock&)> fold;          // its kernel over the block that is in c->d_out4 / c->d_reasons (the
                                                      // driver has run launch_out_stats_accum inside the same timer pair)
  std::function<int(unsigned long long* red)> finish; // its last kernel and its downloads, c->d_red into red[8] among them
                                                      // (select_download_red, or a copy of its own beside what it waits for)
};
// The checks of an entry, in this order, before any output or anything of the context is touched:
//   select_check_shape   the context, the matrix (check_src), ICIKT_TOPK_MAX_SAMPLES (`cap_why`: the entry's reason for it)
//   (the entry's own)    k, rule, max_edges, cls, null outputs
//   select_check_args    perspective, alternative, global_na; then resets max_taumax and reason_counts
// select_budget (n_samp > 0) makes the context's device current and gives the pairs a block may hold (tkblock, else
// kTriangleBlockPairs).  select_run runs the blocks -- a call of one block pipelined by column chunks
// (upload_prepare_pairs), several blocks behind one upload -- then steps.finish, leaves the context without prepared
// state or pair list, and decodes red into max_taumax and reason_counts.
int select_check_shape(const SelectCall& s, const char* cap_why);
int select_check_args(SelectCall& s);
int select_budget(const SelectCall& s, int64_t* budget);
int select_run(SelectCall& s, PairBlocks& blocks, const SelectSteps& steps);
// Steps several entries share, on c->stream; the key planes and the sort's scratch are c->sel's (SelectWork).
// the fold that keeps a block's raw as keys: launch_median_keep into sel.kept at the block's place
int select_keep_raw(icikt_ctx* c, const PairBlock& b);
// the eight words of c->d_red into red, delivered with the call's results (download): a finish's last step
int select_download_red(icikt_ctx* c, unsigned long long* red);
// The stable radix sort of the P keys in `a`, ascending, `a` and `b` ping-ponging, tile keys per wave (padj_tile).
// h_dhist [8][256] is the downloaded digit table of those keys: a digit is skipped iff one of its values holds all P
// keys (the pass would move nothing).  Reserves sel.counts and sel.agg for this P and tile -- agg stays good for the
// scans of the same P behind the sort.  *sorted is the plane that holds the keys in order, *spare the other one.  No
// timer pair: the caller's is around the sort and its own kernels.
int select_sort(icikt_ctx* c, int64_t P, long long tile, const unsigned long long* h_dhist, unsigned long long* a,
                unsigned long long* b, unsigned long long** sorted, unsigned long long** spare);

// ---- class labels, and the labellings of the permutation-test entries (icikt_labels.h holds what needs no device) ----
// every label of `name` [n] (cls, ref_cls, perm_cls[q]) inside 0 .. n_class - 1, `who` prefixing the message
int check_labels(icikt_ctx* c, const char* who, const std::string& name, const int32_t* lab, int64_t n, int64_t n_class);
// cls of an entry (null: one class, nothing is checked): n_class at least 1, at most class_cap (0: no cap; cap_why is
// the entry's reason for it), then check_labels over the call's n_samp
int select_check_classes(const SelectCall& s, const int32_t* cls, int n_class, int class_cap = 0, const char* cap_why = "");
// ... and the permutations behind it: n_perm in 0 .. ICIKT_ANOSIM_MAX_PERM, (1 + n_perm) classes within cell_cap
// (ICIKT_PERMANOVA_MAX_CELLS; 0: no cap), perm_cls where n_perm > 0.  The labels of perm_cls are select_labellings'.
int select_check_labellings(const SelectCall& s, const int32_t* cls, int n_class, int class_cap, const char* cap_why,
                            const int32_t* perm_cls, int64_t n_perm, int64_t cell_cap = 0);
// The labellings of a call with n_samp > 0, made before select_run: the observed one first (a null cls: zeros), then
// the n_perm rows of perm_cls; plan says how many an upload takes (label_batches: bytes_per_lab and the anoperms key).
// Reserves c->labels for a batch.
struct Labellings {
  const int32_t* perm_cls = nullptr;
  int64_t S = 0, n_class = 1, n_lab = 1;
  LabelBatches plan{};
  std::vector<int32_t> obs;      // the observed labelling
  std::vector<uint16_t> stage;   // one batch as the device takes it: [groups][S][ANO_PB]
  std::vector<int64_t> size_of;  // stage_labellings' class sizes
};
int select_labellings_begin(const SelectCall& s, const int32_t* cls, int n_class, const int32_t* perm_cls, int64_t n_perm,
                            int64_t bytes_per_lab, Labellings* L);
// what an entry does per batch, on c->stream
struct LabellingSteps {
  std::function<int(int64_t groups, int64_t nb)> launch;   // its kernels over the nb labellings (`groups` groups of ANO_PB) in
                                                           // c->labels, inside the driver's ICIKT_K_EPILOGUE timer pair
  std::function<int(int64_t q0, int64_t nb)> collect;      // download and wait for the sums of the launched batch, labellings
                                                           // [q0, q0 + nb) of the call
};
// The labellings batch by batch, from an entry's finish step.  Per batch: staged and checked on the host
// (stage_labellings, while the batch before runs: a bad label fails the call as "who: perm_cls[q][s] = v is outside
// ..."), the batch before collected, the stage uploaded (which is what waits for that batch's kernels), steps.launch.
// The last batch is collected at the end.  device == false: the labels are checked all the same, nothing is uploaded,
// launched or collected.  within (optional, [n_lab]): every labelling's pairs of samples that share a class.
int select_labellings(const SelectCall& s, Labellings& L, bool device, int64_t* within, const LabellingSteps& steps);

}  // namespace host
}  // namespace icikt
#endif
