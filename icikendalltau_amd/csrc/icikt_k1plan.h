// icikt_k1plan.h -- the pair kernel's launch plan (k1_pairs): the LDS layout and the option word the
// kernel and the plan share, the plan itself (plan_k1), the verdict on the prepared columns' tie structure (tie_verdict),
// the task list (combn_pairs, build_units), its slices by column chunk for the pipelined host entries (combn_chunk_units,
// order_units_by_chunk) and the grid of a launch (k1_grid).  Host arithmetic only: no device header,
// so tests/k1plan_print.cpp compiles it with the host compiler alone (tests/test_k1plan_host.py).  Part of
// icikt_device.h -- the shared layout keeps its __host__ __device__ there through ICIKT_HD -- and of icikt_host.h;
// icikt_pipeline.cpp holds the callers, which fill the context, talk to the device and print the verbose lines.
#ifndef ICIKT_K1PLAN_H
#define ICIKT_K1PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define ICIKT_HD __host__ __device__
#else
#define ICIKT_HD
#endif

namespace icikt {

// Per-column result of the pre-pass (K0).
struct ColStats {
  int32_t nna;       // missing rows
  int32_t ngroups;   // distinct values after the fill (unique(), kendallc.cpp:234-235)
  int32_t tfill;     // size of the fill group (missing rows + rows equal to min-0.1); 0 if nna == 0
  int32_t maxgroup;  // largest tie group: size << 16 | its first ascending position
  uint32_t s0, s1, s2;  // count_rank_tie sums in wrapping int32: t(t-1), t(t-1)(t-2), t(t-1)(2t+5)
  uint32_t ntg;      // tie groups of size >= 2 (length of the column's tgroups list)
  long long e0, e1, e2;  // the same sums exactly
  double fill;           // min - 0.1
  int32_t nexcl;         // rows excluded by the caller's global_na rule (MaskSpec): exclude_loc of R/utils.R:1-23.
                         // == nna unless the data hold NaN and NaN is not in global_na
  int32_t flags;         // bit 0 COL_ODD_TIE: some tie group of >= 2 rows starts at an ODD ascending position;
                         // bits 8..31: what STREAMING the column costs a pair kernel task, in half hot steps (2 per 64-row hot
                         // step, 3 per MIXED / SOLO / GROUP step): the cost-weighted pair blocks of the multi-device driver
};

// bytes of a counter of count mode (k1_pairs): 2 -- two to a dword, twice the tie groups per LDS byte -- or 4 (a build
// option for measurements: -DICIKT_CNT_BYTES=4)
#ifndef ICIKT_CNT_BYTES
#define ICIKT_CNT_BYTES 2
#endif
static_assert(ICIKT_CNT_BYTES == 2 || ICIKT_CNT_BYTES == 4, "counter width");

// one pair per wave: bytes of the counts of `seen` (loc 64 x 16 x u8, lb 64 x u32, hist 64 x u32, locg 64 x 4 x u16)
constexpr int K1_TL_BYTES = 1024 + 256 + 256 + 512 + 64;   // (+ 64: the closed-form tail reuses the area as a u16 prefix over Wp <= 1 025 words)

// half-wave kernels: bytes of a pair's prefix slots (32 lanes x one aligned slot of 8 u16 -- 16 u16 above 8 words per
// lane)
ICIKT_HD inline int k1_half_pre(int half_items) { return 32 * (half_items > 8 ? 16 : 8) * 2; }

// half-wave K1 kernels exist for 1..7, 9, 11, 13 and 15 words per lane of a half's prefix rebuild: n <= 30 656 (the packed
// in-step compares of those kernels need positions -- the guard position 64 W included -- below 2^15).  An EVEN number of
// words per lane from 8 on puts the lanes' words at a stride of 64 / 128 bytes, an 8- / 16-way LDS bank conflict per read
// (8 words measured at half the speed of one pair per wave), so such columns run the next odd kernel.  (Round 2 measured
// 11 and 13 words per lane at 2 waves per SIMD -- the LDS state with `pend` allowed no more -- and did not keep them;
// without `pend` they run 4 waves per SIMD.)
constexpr int ICIKT_HALF_ITEMS_MAX = 15;
ICIKT_HD inline int k1_half_items(int Wp) {
  const int hi = (Wp + 31) >> 5;
  return (hi >= 8 && (hi & 1) == 0) ? hi + 1 : hi;
}

// Stride (in 64-bit words) of a pair's LDS / pend arrays in K1, shared by the kernel and the host plan.  The
// arrays are padded so that the hot steps' prefix rebuilds run without predicates:
//  * half-wave kernels: 32 lanes x half_items words;
//  * one pair per wave: the Wp words, rounded up to a multiple of 8 (two words are read at a time, and the u16 array
//    `ppre` of that length must end on a 16-byte boundary; an owner of the two-level counts has 16 words whatever the
//    length, and the owners past the last word own nothing).
ICIKT_HD inline int k1_lds_stride(int Wp, int half_items) {
  if (half_items > 0) return 32 * half_items;
  return (Wp + 7) & ~7;
}

// The pair kernel's option word (`opts` of launch_k1 and k1_pairs; one int as a kernel argument): packed by the host's
// launch plan (plan_k1 and k1_grid below), read by the kernel, both through the names below
// (a flag is tested as `opts & K1_OPT_...`, a field read through its accessor).
constexpr int K1_OPT_HALF = 1;          // bit 0: half-wave hot step (one pair per 32-lane half, 32-row sub-steps)
constexpr int K1_OPT_ROW_ONLY = 2;      // bit 1: row mode only (joint ties of a long group neither from a list nor from counters)
constexpr int K1_OPT_HALF_LAYOUT = 4;   // bit 2: two long-column pairs of a whole-wave kernel take the singleton region in the
                                        // half layout (one pair per 32-lane half, 32-row sub-steps, the half-wave in-step chain)
constexpr int K1_OPT_NO_SOLO = 8;       // bit 3: no SOLO steps
constexpr int K1_OPT_SEG_SHIFT = 4;     // bits 4..5: log2 of the segments a half-wave task is cut in (1, 2 or 4)
constexpr int K1_OPT_LIST_SHIFT = 8, K1_OPT_LIST_MASK = 0x3FF;   // bits 8..17: list mode's reach, in tie groups of the gathered column
constexpr int K1_OPT_CNT_SHIFT = 18;    // bits 18 and up: entries of a pair's counter table (count mode); 0: none
ICIKT_HD constexpr int k1_opt_segments(int opts) { return 1 << ((opts >> K1_OPT_SEG_SHIFT) & 3); }
ICIKT_HD constexpr int k1_opt_tg_list(int opts) { return (opts >> K1_OPT_LIST_SHIFT) & K1_OPT_LIST_MASK; }
ICIKT_HD constexpr int k1_opt_cnt_cap(int opts) { return opts >> K1_OPT_CNT_SHIFT; }
ICIKT_HD constexpr int k1_opt_pack_segments(int split) { return (split == 4 ? 2 : split == 2 ? 1 : 0) << K1_OPT_SEG_SHIFT; }
ICIKT_HD constexpr int k1_opt_pack_tg_list(int tg_list) { return tg_list << K1_OPT_LIST_SHIFT; }
ICIKT_HD constexpr int k1_opt_pack_cnt_cap(int entries) { return entries << K1_OPT_CNT_SHIFT; }

namespace host {

// launch-plan overrides of the pair kernel (icikt_debug_set_plan; -1 = the library's choice)
struct PlanOverride {
  int np = -1, wpb = -1, half = -1, grid_mult = -1, grid_cap = -1, hyb = -1;
  bool has_tgmax = false;
  int tgmax = 0;
  int waves = -1;     // half-wave kernels: waves per CU the counter tables may cost the launch down to (default: none)
  int merge = -1;     // pipelined host entries: 1 = the pairs in ONE launch behind the last chunk, 0 = a launch per chunk, whatever the pair count
  int split = -1;     // half-wave kernels: segments per task (1 | 2 | 4), whatever the launch's size
  int solo = -1;      // 0: SOLO steps of the tie program run as MIXED steps (with the in-step chains)
  int list = -1;      // list mode (range counts per listed tie group) up to this many tie groups: count mode takes over above
  long long tkblock = -1;   // icikt_topk_*, icikt_edges_*, icikt_class_medians_*, icikt_quantiles_*: pairs a block (whole combn rows, or a slice of the class list) may hold (default: the library's budget)
  int medlds = -1;          // icikt_class_medians_*, icikt_class_matrix_*: partners up to which the select kernel gathers a sample's keys into LDS (default: MEDIAN_STAGE_MAX)
  int qbatch = -1;          // icikt_quantiles_*: targets the select runs per batch (default: QUANT_BATCH_MAX)
  long long padjtile = -1;  // icikt_padjust_*, icikt_anosim_*: keys of a wave's tile of the sort (default: padj_tile's choice)
  long long anoperms = -1;  // icikt_anosim_*: labellings per upload (default: ANO_BATCH_BYTES of labels)
  int anostrip = -1;        // icikt_anosim_*: columns of a workgroup of the permutation kernel (default: ANO_STRIP_DEFAULT)
  int hcgrid = -1;          // icikt_hclust_*: workgroups of the rescan kernel (default: min(S, HCLUST_GRID_MAX))
  bool verbose = false;
};

// launch plan of the pair kernel for a given n
struct K1Plan {
  int np;            // pairs per wave: 2 (one per half, consecutive pairs with the same pi) or 1
  int wpb;           // waves per workgroup
  size_t lds_bytes;
  int perpair_bytes;
  int opts;          // the pair kernel's option word (K1_OPT_* above)
  int half_items;    // words per lane of a half-wave prefix rebuild (0: no half-wave step)
  int stride;        // 64-bit words between a pair's LDS / pend arrays (k1_lds_stride)
  int split;         // half-wave kernels: segments a task is cut in (1 | 2 | 4) when the task list leaves the chip half empty
};

// n, Wp: rows and bitset words (W + 1) of a prepared column (PrepView)
inline K1Plan plan_k1(int n, int Wp, int64_t n_pairs, int n_cu, const PlanOverride& ov, bool tied, int ntg_hint = -1, int group_hint = 0) {
  K1Plan pl{};
  const size_t lds_cap = 160 * 1024;
  // n <= 18 336 (a half wave rebuilds a prefix with <= 9 words per lane): two pairs per wave, one per 32-lane half.
  // Longer columns: pairs on the whole wave -- TWO per wave, one after the other, while eight waves of two pairs fit a
  // CU's LDS (n <~ 60 000), else one.  The two share the streamed column and the rec block, so one 8-byte gather per row
  // serves both: the pair kernel of long columns was bound by the L2's request rate (64 requests per wave and gather; the
  // block never sits in an L1), not by instruction issue (round 3: a quarter fewer vector instructions changed nothing
  // at n = 50 000).  Measured (tools/n_sweep.py, 512 columns, one pair -> two pairs per wave -> their singleton region in
  // the half layout): n = 20 000 1.24e7 -> 1.69e7 -> 1.98e7 pairs/s, 30 000 8.0e6 -> 1.13e7 -> 1.33e7, 36 000 6.6e6 -> 9.4e6
  // -> 1.11e7, 50 000 4.9e6 -> 5.8e6 -> 7.2e6, 60 000 4.1e6 -> 4.9e6 -> 6.0e6, 65 535 3.7e6 -> 3.9e6 -> 4.6e6.
  // No kernel keeps a second bitset for open tie groups any more (`pend`, in LDS or in per-wave global slots with a
  // persistent grid: rounds 1-2): the plan key pend of icikt_debug_set_plan is accepted and ignored.
  // 18 337 .. 30 656 rows: BOTH families fit.  Continuous columns run 25-50 % faster in the long-column kernel (n = 20 000:
  // 1.98e7 vs 1.55e7 pairs/s; 30 000: 1.33e7 vs 0.88e7: the half-wave prefix rebuild costs 11 .. 15 words per lane there,
  // the long-column kernel takes singleton rows in the half layout over the two-level counts: K1_OPT_HALF_LAYOUT below),
  // tied columns 1.4-2.1x faster in the half-wave kernels (their MIXED steps use the packed chains and the pre-pass's
  // masks; n = 30 000, ~15 000 / 3 000 / 600 distinct values: 1.48 / 1.95 / 1.74 ms vs 2.46 / 4.12 / 2.83): `tied` (the
  // prepared columns average more than eight tie groups: tie_verdict below) chooses.
  const bool half_fits = icikt::k1_half_items(Wp) <= icikt::ICIKT_HALF_ITEMS_MAX;
  // (15 200 .. 18 336 rows, the upper part of nine words per lane: the same choice, for less -- continuous columns 3-5 % faster in
  //  the long-column kernel, n = 16 000: 2.48e7 vs 2.38e7 pairs/s, 18 336: 2.07e7 vs 1.97e7; level at 14 400)
  const int hi_words = icikt::k1_half_items(Wp);
  const bool both_fit = hi_words > 9 || (hi_words == 9 && n >= 15200 && n_pairs > (int64_t)4 * n_cu);   // (a short task list: the half-wave kernels, cut in segments)
  const bool half_ok = half_fits && (!both_fit || (ov.half < 0 ? tied : ov.half != 0));
  int np = half_ok ? 2 : 1;
  {
    const size_t two = 2 * ((size_t)icikt::k1_lds_stride(Wp, 0) * 8 + icikt::K1_TL_BYTES);
    if (!half_ok && 7 * two <= lds_cap) np = 2;   // (65 535 rows: seven single-wave workgroups, 3.96e6 vs 3.74e6)
  }
  // few pairs: twice the waves hide the latency of a step better than two pairs per wave share their loads while
  // the chip is nearly empty (measured on the yeast matrix cut to 24 .. 96 columns: one pair per wave wins up to
  // 780 pairs, 0.209 vs 0.230 ms, two pairs per wave from 1 128 pairs on, 0.231 vs 0.242 ms)
  // (round 4, last change: that held for the tie steps of round 3.  With step records, count mode and SOLO steps the
  //  half-wave kernels win at every size on tied data -- yeast cut to 4 .. 32 columns: 0.13 against 0.22 ms -- and draw level
  //  on continuous data, 0.08 against 0.07 ms at 10 000 x 8 .. 32: only the whole-wave family still drops to one pair per wave)
  if (n_pairs <= (int64_t)4 * n_cu && !half_ok) np = 1;
  // columns too long for the half-wave kernels whose tie groups are many and short (tie_verdict): one pair per wave
  if (tied && !half_fits) np = 1;
  // overrides for experiments and tests (icikt_debug_set_plan; the product path reads no environment variable)
  if (ov.np == 1 || ov.np == 2) np = ov.np;
  int wpb = 4;
  if (!half_ok && np == 2) {   // fewer than two four-wave workgroups of two pairs fit: single-wave workgroups fill the LDS
    const size_t two = 2 * ((size_t)icikt::k1_lds_stride(Wp, 0) * 8 + icikt::K1_TL_BYTES);
    if (8 * two > lds_cap) wpb = 1;
  }
  if (ov.wpb > 0) wpb = std::max(1, std::min(8, ov.wpb));
  pl.opts = icikt::K1_OPT_HALF;
  if (ov.half >= 0 && !both_fit) pl.opts = ov.half ? icikt::K1_OPT_HALF : 0;
  int tg_max = 128;  // whole-wave kernels: joint ties of a closing group from the gathered column's tie-group list
                     // while it has at most this many groups (the kernels cap it at 128: two listed groups per lane), else row
                     // by row; half-wave kernels: the entries of a pair's counter table (count mode), sized below
  if (ov.has_tgmax) tg_max = std::max(-1, std::min(1 << 20, ov.tgmax));
  const bool row_only = tg_max < 0;
  if (row_only) { pl.opts |= icikt::K1_OPT_ROW_ONLY; tg_max = 0; }
  // list mode (range counts per listed tie group at a group's close: a cost per CLOSE, right for few, long
  // groups -- and same-address atomics of count mode would serialise there) up to this many tie groups
  int tg_list = std::min(tg_max, 128);   // (raised to 256 below for the half-wave kernels of 11 .. 15 words per lane)
  // half-wave kernels: a half rebuilds a prefix with half_items words per lane, unpredicated, so the LDS arrays of such
  // a kernel are padded to 32 * half_items words; every other plan runs pairs on the whole wave
  pl.half_items = icikt::k1_half_items(Wp);
  if (np != 2 || !half_ok || !(pl.opts & icikt::K1_OPT_HALF)) {
    pl.opts &= ~icikt::K1_OPT_HALF;
    pl.half_items = 0;
  }
  // two long-column pairs of a whole-wave kernel take the singleton region in the half layout (one pair per
  // 32-lane half, 32-row sub-steps, the half-wave in-step chain)
  if (np == 2 && pl.half_items == 0 && ov.hyb != 0) pl.opts |= icikt::K1_OPT_HALF_LAYOUT;
  // final layout: the kernel derives the same stride from (Wp, half_items)
  pl.stride = icikt::k1_lds_stride(Wp, pl.half_items);
  if (pl.half_items > 0) {
    // seen + prefix slots + the counters of count mode: one u16 per tie group of a gathered column (+ one for the rows
    // that are their own group), as many as the LDS holds WITHOUT costing the launch a wave it would otherwise run: six
    // waves per SIMD (five from 11 words per lane on) or, for a short task list, the waves the list fills
    const size_t base = (size_t)pl.stride * 8 + icikt::k1_half_pre(pl.half_items);
    auto pair_bytes = [&](int cap) { return (base + ICIKT_CNT_BYTES * ((size_t)cap + 2) + 15) & ~(size_t)15; };
    auto waves_fit = [&](int cap) { return (int)(lds_cap / ((size_t)wpb * np * pair_bytes(cap))) * wpb; };
    const int waves_max = 4 * (pl.half_items > 9 ? 5 : 6);
    const int64_t tasks = (n_pairs + 1) / 2;
    // a task list that leaves the chip half empty: every task is cut in 2 or 4 segments, a wave each (k1_pairs) -- such a
    // launch lasts as long as ONE task otherwise; the counter tables are then sized for the waves of the segments
    // (measured on yeast columns and 10 000-row synthetic ones, 4 .. 96 columns: four segments pay while the segments' waves
    //  number at most the chip's SIMDs, two up to 2.5 tasks per CU; beyond, the launch is bound by the SIMDs that hold three waves,
    //  not by a wave's latency, and the rows inserted twice only add work -- the full yeast matrix: 0.208 -> 0.237 ms)
    pl.split = 1;
    if (n >= 2048) pl.split = (tasks <= (int64_t)n_cu) ? 4 : (2 * tasks <= (int64_t)5 * n_cu) ? 2 : 1;
    if (ov.split == 1 || ov.split == 2 || ov.split == 4) pl.split = ov.split;
    const int waves_needed = (int)std::min<int64_t>(waves_max, std::max<int64_t>(wpb, (tasks * pl.split + n_cu - 1) / std::max(1, n_cu)));
    int waves_target = std::min(waves_needed, std::max(wpb, waves_fit(0)));
    if (ov.waves > 0) waves_target = std::min(waves_target, std::max(wpb, ov.waves));
    const int tg_list_max = row_only ? 0 : (pl.half_items > 9 ? 256 : 128);   // (list mode's reach in this kernel, below)
    int cap = 0;
    if (!row_only) {
      static const int caps[] = {4094, 3072, 2048, 1536, 1024, 768, 512, 384, 256, 192, 128, 64};
      for (int cc : caps) {
        if (cc > n / 2 + 64 && cc > 64) continue;              // (a column of n rows has at most n / 2 tie groups)
        if (waves_fit(cc) >= waves_target) { cap = cc; break; }
      }
      // Columns of 14 273 rows and more leave the tables next to nothing at that occupancy (15 words per lane: 64 counters
      // beside 4.9 KB of state per pair).  When the prepared columns' statistics (tie_verdict: read back once per matrix at
      // these lengths) say that their tie groups would fit a table at three waves per SIMD, the table is worth the waves:
      // count data -- negative binomial, ~700 tie groups per column, nine rows in ten in groups of more than 32 -- 20 000 x
      // 256: 4.2 -> 3.2 ms, 30 000 x 256: 6.8 -> 4.7 (row mode streams a long group three times).
      // (... when list mode cannot serve them and a tied pair of rows sits, on average, in a group of 256 rows or more -- from the
      //  columns' tie sums, fill group apart: 30 000-row columns of 600 tie groups of ~100 rows run 1.61 ms in row mode at four waves
      //  per SIMD, 1.98 in count mode at three)
      if (ntg_hint > std::max(cap, tg_list_max) && group_hint >= 256 && ov.waves <= 0 && pl.half_items >= 9) {
        for (int i = (int)(sizeof(caps) / sizeof(caps[0])) - 1; i >= 0; --i) {
          if (caps[i] < ntg_hint) continue;
          if (waves_fit(caps[i]) >= 12) cap = caps[i];
          break;
        }
      }
      if (ov.has_tgmax) cap = std::min(cap, tg_max);
    }
    tg_max = cap;
    pl.perpair_bytes = (int)pair_bytes(cap);
  } else {
    // seen + the two-level counts + the counters of count mode (round 4: the whole-wave kernels too): as many as the LDS holds
    // beside the waves the launch runs anyway -- 50 000 rows: 512 counters per pair at eight waves of two pairs (or sixteen of one)
    const size_t base = (size_t)pl.stride * 8 + icikt::K1_TL_BYTES;
    auto pair_bytes = [&](int cap) { return cap > 0 ? ((base + ICIKT_CNT_BYTES * ((size_t)cap + 2) + 15) & ~(size_t)15) : base; };
    auto waves_of = [&](size_t pb, int w0) {   // waves a CU holds with pb bytes per pair in workgroups of up to w0 waves
      const int w = std::max(1, std::min(w0, (int)(lds_cap / (pb * np))));
      return (int)(lds_cap / ((size_t)w * np * pb)) * w;
    };
    auto waves_any = [&](size_t pb) { return std::max(waves_of(pb, wpb), waves_of(pb, 1)); };   // (single-wave workgroups pack the LDS best)
    int cap = 0;
    if (!row_only && !ov.has_tgmax) {
      static const int caps[] = {4094, 3072, 2048, 1536, 1024, 768, 512, 384, 256};
      const int target = std::min(waves_of(base, wpb), np == 2 ? 12 : 24);   // (the registers' limit: 3 / 6 waves per SIMD)
      for (int cc : caps) {
        if (cc > n / 2 + 64) continue;                     // (a column of n rows has at most n / 2 tie groups)
        if (waves_any(pair_bytes(cc)) >= target) { cap = cc; break; }
      }
      // the prepared columns hold more tie groups than that (tie_verdict's read-back): a table that covers them is worth one wave
      // of eight -- count-like data, 50 000 x 96, ~630 tie groups per column (at most 940): 2.76 ms with 512 counters at eight
      // waves per CU, 2.48 with 1 024 at seven
      // (... when a tied pair of rows sits, on average, in a group of 256 rows or more: groups of one or two steps close from
      //  registers in row mode, for less than the counters and the lost wave cost -- 50 000 x 128 columns of ~1 000 tie groups of
      //  ~120 rows: 5.24 ms in row mode, 5.77 with the table)
      if (ntg_hint > cap && group_hint >= 256 && target >= 6) {
        for (int i = (int)(sizeof(caps) / sizeof(caps[0])) - 1; i >= 0; --i) {
          if (caps[i] < ntg_hint) continue;
          if (waves_any(pair_bytes(caps[i])) >= target - 1) cap = caps[i];
          break;
        }
      }
      if (cap > 0 && ov.wpb <= 0 && waves_of(pair_bytes(cap), 1) > waves_of(pair_bytes(cap), wpb)) wpb = 1;
    } else if (!row_only && ov.tgmax > 128) {
      cap = std::min(ov.tgmax, 4094);   // (tests: a table whatever it costs in waves)
      while (cap > 0 && pair_bytes(cap) * np > lds_cap) cap /= 2;
    }
    pl.perpair_bytes = (int)pair_bytes(cap);
    pl.opts |= icikt::k1_opt_pack_cnt_cap(cap);   // entries of a pair's counter table (count mode); 0: none
  }
  // (eight listed groups per lane in the kernels that have the registers: list mode up to 256 tie groups there -- count
  //  mode has 64 counters beside their 4.9 KB of LDS state per pair, and row mode streams a long group three times)
  if (pl.half_items > 9 && !row_only) tg_list = std::min(ov.has_tgmax ? std::max(0, ov.tgmax) : 256, 256);
  if (ov.list >= 0) tg_list = std::min(tg_list, ov.list);
  pl.opts |= icikt::k1_opt_pack_tg_list(tg_list);
  if (ov.solo == 0) pl.opts |= icikt::K1_OPT_NO_SOLO;
  if (pl.half_items > 0) pl.opts |= icikt::k1_opt_pack_cnt_cap(tg_max);   // entries of a pair's counter table (count mode)
  const int fit = std::max(1, (int)(lds_cap / ((size_t)pl.perpair_bytes * np)));
  pl.np = np;
  pl.wpb = std::min(wpb, fit);
  pl.lds_bytes = (size_t)pl.wpb * np * pl.perpair_bytes;
  return pl;
}

// Do the prepared columns hold tie groups beyond a fill group or so?  Only asked where the answer chooses the kernel:
// 15 200 .. 30 656 rows (the kernel family), and longer columns (pairs per wave: columns of many SHORT tie groups -- on
// average fewer than 32 rows per group -- run their tie steps one pair after the other whatever shares the wave, and one
// pair per wave then has twice the waves to hide a step's latency: 50 000 x 512 columns of ~10-row groups 123 -> 88 ms;
// columns of long groups share their gathers and keep two pairs per wave, 75 against 113 ms).  st: the statistics of the
// columns read back (matrix_tied, icikt_pipeline.cpp: up to 64 of them, once per prepared matrix) of n rows each; long_cols:
// too long for the half-wave kernels.
struct TieVerdict {
  int tied_state, ntg_hint, group_hint;          // as icikt_ctx keeps them (icikt_host.h)
  unsigned long long groups, all_groups, rows;   // the columns' sums behind the verdict (the verbose line)
};
inline TieVerdict tie_verdict(const std::vector<ColStats>& st, int n, bool long_cols) {
  TieVerdict v{};
  const unsigned long long m = st.size();
  unsigned long long groups = 0, all_groups = 0, rows = 0;
  double g0 = 0.0, g1 = 0.0;
  for (const auto& t : st) {
    groups += t.ntg;
    v.ntg_hint = std::max(v.ntg_hint, (int)std::min<uint32_t>(t.ntg, 1u << 20));
    // the size of the tie group a random tied PAIR of rows sits in, fill group apart: sum t (t-1) (t-2) / sum t (t-1) + 2
    {
      const long long f = t.tfill;
      g0 += (double)(t.e0 - f * (f - 1));
      g1 += (double)(t.e1 - f * (f - 1) * (f - 2));
    }
    all_groups += (unsigned long long)std::max(t.ngroups, 1);
    rows += (unsigned long long)std::max(0, n - t.nna);
  }
  v.group_hint = (g0 > 0.0) ? (int)std::min(1.0e6, g1 / g0 + 2.0) : 0;
  const bool tied = groups > 8ull * m;
  v.tied_state = (tied && (!long_cols || rows < 32ull * all_groups)) ? 1 : 0;
  v.groups = groups, v.all_groups = all_groups, v.rows = rows;
  return v;
}

// Tasks (one wave each), as (pair index, pair index or -1).  np == 1: one pair per task.  np == 2: two pairs
// that share their streamed column pj and whose gathered columns pi are the two columns (2a, 2a+1) of one
// block of the interleaved rec table, so that ONE 8-byte gather per row serves both pairs; pairs without such
// a partner run alone.  Tasks are ordered by gathered block, then streamed column (cache locality of the
// block's rec table).
// the host copies of the combn range [begin, end) of combn(n_samp, 2) (the device arrays were filled by a kernel)
inline void combn_pairs(int64_t n_samp, int64_t begin, int64_t end, std::vector<int32_t>& h_pi, std::vector<int32_t>& h_pj) {
  h_pi.resize((size_t)(end - begin));
  h_pj.resize((size_t)(end - begin));
  // walk combn order: row i holds pairs (i, i+1..S-1), starting at offset i*S - i(i+1)/2
  int64_t i = 0, row_start = 0;
  while (i < n_samp - 1 && row_start + (n_samp - 1 - i) <= begin) {
    row_start += n_samp - 1 - i;
    ++i;
  }
  int64_t j = i + 1 + (begin - row_start);
  for (int64_t p = begin; p < end; ++p) {
    h_pi[(size_t)(p - begin)] = (int32_t)i;
    h_pj[(size_t)(p - begin)] = (int32_t)j;
    if (++j >= n_samp) {
      ++i;
      j = i + 1;
    }
  }
}

// the task list u of the pairs (h_pi[p], h_pj[p]), p < P, for np pairs per wave
inline void build_units(const std::vector<int32_t>& h_pi, const std::vector<int32_t>& h_pj, int64_t P, int np, std::vector<int32_t>& u) {
  u.clear();
  const int32_t* pi = h_pi.data();
  const int32_t* pj = h_pj.data();
  u.reserve((size_t)P * 2);
  auto push = [&u](int64_t a, int64_t b) { u.push_back((int32_t)a); u.push_back((int32_t)b); };
  if (np == 1) {
    for (int64_t p = 0; p < P; ++p) push(p, -1);
  } else {
    // combn ranges and setup_comparisons lists are sorted by (pi, pj): merge the rows 2a and 2a+1 on pj
    bool sorted = true;
    for (int64_t p = 1; p < P && sorted; ++p)
      sorted = (pi[p] > pi[p - 1]) || (pi[p] == pi[p - 1] && pj[p] > pj[p - 1]);
    if (sorted) {
      int64_t a = 0;
      while (a < P) {
        int64_t ae = a;
        while (ae < P && pi[ae] == pi[a]) ++ae;
        if ((pi[a] & 1) == 0 && ae < P && pi[ae] == pi[a] + 1) {
          int64_t be = ae;
          while (be < P && pi[be] == pi[ae]) ++be;
          int64_t x = a, y = ae;
          while (x < ae || y < be) {
            if (x < ae && y < be && pj[x] == pj[y]) { push(x, y); ++x; ++y; }
            else if (y >= be || (x < ae && pj[x] < pj[y])) { push(x, -1); ++x; }
            else { push(y, -1); ++y; }
          }
          a = be;
        } else {
          for (int64_t x = a; x < ae; ++x) push(x, -1);
          a = ae;
        }
      }
    } else {
      // any other list: order the pairs by (block of pi, pj, parity of pi) and pair up neighbours
      std::vector<int64_t> idx((size_t)P);
      for (int64_t p = 0; p < P; ++p) idx[(size_t)p] = p;
      auto key = [pi, pj](int64_t p) {
        return ((uint64_t)(uint32_t)(pi[p] >> 1) << 33) | ((uint64_t)(uint32_t)pj[p] << 1) | (uint64_t)(pi[p] & 1);
      };
      std::sort(idx.begin(), idx.end(), [&key](int64_t x, int64_t y) {
        const uint64_t kx = key(x), ky = key(y);
        return kx < ky || (kx == ky && x < y);
      });
      int64_t i = 0;
      while (i < P) {
        const int64_t x = idx[(size_t)i];
        if (i + 1 < P) {
          const int64_t y = idx[(size_t)i + 1];
          if ((pi[x] & 1) == 0 && pi[y] == pi[x] + 1 && pj[y] == pj[x]) { push(x, y); i += 2; continue; }
        }
        push(x, -1);
        ++i;
      }
    }
  }
}

// The pipelined host entries launch the pair kernel once per column chunk, over the tasks whose LAST column arrived
// with that chunk.  Two producers of those slices, one rule -- for the full triangle they give the same lists
// (tests/test_k1plan_host.py):

// All pairs of the upper triangle of S columns: a chunk's tasks are arithmetic.  The tasks whose last column lies in
// [cb, ce), as (p0, p1 | -1), written at u (the caller's pinned staging buffer: no host copy of the pair list is ever
// made); returns their count.  Order inside a chunk: gathered block, then streamed column (the order build_units gives:
// a block's rec table stays in cache); np == 2: a task is the two pairs (2a, j), (2a + 1, j) that share their streamed
// column j, the pair (2a, 2a + 1) runs alone; np == 1: i, then j.
inline size_t combn_chunk_units(int64_t S, int64_t cb, int64_t ce, int np, int32_t* u) {
  auto pidx = [S](int64_t i, int64_t j) { return (int32_t)(i * (2 * S - i - 1) / 2 + (j - i - 1)); };
  size_t nt = 0;
  if (np == 2) {
    for (int64_t a2 = 0; a2 < ce; a2 += 2) {          // gathered block: columns a2, a2 + 1
      const int64_t c1 = a2 + 1;
      for (int64_t j = std::max(cb, a2 + 1); j < ce; ++j) {
        if (j == c1) { u[2 * nt] = pidx(a2, c1); u[2 * nt + 1] = -1; }
        else { u[2 * nt] = pidx(a2, j); u[2 * nt + 1] = pidx(c1, j); }
        ++nt;
      }
    }
  } else {
    for (int64_t i = 0; i < ce; ++i)
      for (int64_t j = std::max(cb, i + 1); j < ce; ++j) { u[2 * nt] = pidx(i, j); u[2 * nt + 1] = -1; ++nt; }
  }
  return nt;
}

// Any pair list (pi[p], pj[p]): its task list `units` (build_units) reordered by the chunk of a task's last column
// (a stable counting sort: inside a chunk the cache-friendly order stays).  Columns [.., chunk_col_end[q]) have arrived
// with chunk q; the tasks of chunk q end up at [first[q], first[q + 1]) -- first has nchunks + 1 entries.
inline void order_units_by_chunk(std::vector<int32_t>& units, const int32_t* pi, const int32_t* pj,
                                 const std::vector<int64_t>& chunk_col_end, std::vector<int>& first) {
  const size_t nchunks = chunk_col_end.size();
  first.assign(nchunks + 1, 0);
  if (nchunks == 0) return;
  const int T = (int)(units.size() / 2);
  std::vector<int32_t> col_chunk((size_t)std::max<int64_t>(chunk_col_end.back(), 0), 0);
  size_t k = 0;
  for (size_t col = 0; col < col_chunk.size(); ++col) {
    while (k + 1 < nchunks && (int64_t)col >= chunk_col_end[k]) ++k;
    col_chunk[col] = (int32_t)k;
  }
  std::vector<int32_t> tchunk((size_t)T);
  for (int t = 0; t < T; ++t) {
    const int32_t p0 = units[2 * (size_t)t], p1 = units[2 * (size_t)t + 1];
    int32_t col = std::max(pi[p0], pj[p0]);
    if (p1 >= 0) col = std::max(col, std::max(pi[p1], pj[p1]));
    tchunk[(size_t)t] = (size_t)col < col_chunk.size() ? col_chunk[(size_t)col] : (int32_t)(nchunks - 1);
    first[(size_t)tchunk[(size_t)t] + 1] += 1;
  }
  for (size_t q = 0; q < nchunks; ++q) first[q + 1] += first[q];
  std::vector<int> fill(first.begin(), first.end() - 1);
  std::vector<int32_t> sorted((size_t)T * 2);
  for (int t = 0; t < T; ++t) {
    const int d = fill[(size_t)tchunk[(size_t)t]]++;
    sorted[2 * (size_t)d] = units[2 * (size_t)t];
    sorted[2 * (size_t)d + 1] = units[2 * (size_t)t + 1];
  }
  units.swap(sorted);
}

// The grid of one launch of the pair kernel over `count` tasks.
// Half-wave kernels: every wave takes one task (grid = all tasks; workgroups start in order, and the kernel's XCD-aware
// block mapping keeps the tasks of one gathered block on one XCD's L2): measured 9 % faster on c4 than persistent
// waves, which run in lockstep and end on a ragged last round.  Whole-wave kernels (long columns, few and long
// tasks per CU): when the task list is longer than what the chip holds, the grid is what the chip holds and the waves
// FETCH their tasks, in order, from one counter per XCD group (k1_pairs: why the order matters for the L2) -- a wave
// that has finished goes on at once instead of waiting for the other waves of its workgroup to retire (c5: +2.4 %).
// Half-wave kernels, a task list that leaves the chip half empty: every task is cut in 2 or 4 segments (k1_pairs), a wave
// each -- such a launch lasts as long as ONE task otherwise.  The segments add their counts up: the pairs' records are
// cleared first.
// -> segments per task, the option word with them packed in, workgroups, and whether the waves fetch their tasks;
// per_cu: workgroups of the plan's kernel a CU holds (whole-wave plans; >= 1); grid_mult, grid_cap: the plan keys
struct K1Grid { int split, opts, blocks; bool persistent; };
inline K1Grid k1_grid(const K1Plan& pl, int count, int per_cu, int n_cu, int grid_mult, int grid_cap) {
  int split = 1, opts = pl.opts;
  if (pl.half_items > 0 && pl.np == 2 && pl.split > 1) {
    split = pl.split;
    opts |= icikt::k1_opt_pack_segments(split);
  }
  const int want = (int)(((int64_t)count * split + pl.wpb - 1) / pl.wpb);
  int blocks = std::max(1, want);
  bool persistent = false;
  if (pl.half_items == 0) {
    const int64_t resident = (int64_t)per_cu * n_cu;
    const int64_t mult = grid_mult > 0 ? grid_mult : 1;
    int64_t cap = mult * resident;
    // test hook: a grid far smaller than the task list makes every persistent wave run many tasks in a row (the per-XCD
    // task counters, the in-order fetch, the re-initialisation of a wave's LDS state) whatever the chip would hold
    if (grid_cap > 0) cap = std::min<int64_t>(cap, grid_cap);
    if (want > cap) {
      blocks = (int)std::max<int64_t>(cap, 1);
      persistent = true;
    }
  }
  return K1Grid{split, opts, blocks, persistent};
}

}  // namespace host
}  // namespace icikt
#endif
