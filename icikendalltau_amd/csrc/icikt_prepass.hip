// icikt_prepass.hip -- K0, the per-column pre-pass of the ICI-Kendall-tau engine (gfx950, wave64).
//
//   k0_prepare_{large,large8,wide,small,pair}   one workgroup per column: NA bitset, fill = min - 0.1, stable sort (bitonic:
//                    register, lane and LDS stages), tie groups, tie sums, and the column's TIE PROGRAM -- the steps a
//                    half-wave pair kernel takes through it (entry layout and sizes: TPROG_* of icikt_device.h).
//                    Replaces the two std::stable_sort calls per PAIR (kendallc.cpp:247,254) by one sort per COLUMN.
//   k0_expand        rebuilds rec / hirow / girow / tgroups / the tie program from order + meta (what ranks exchange)
//   k0_mask          the mask-only pre-pass of pairwise_completeness
// and their launchers.  The pair kernels (icikt_kernels.hip) read what this unit writes through PrepView.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "icikt_device.h"
#include "icikt_wave.h"

namespace icikt {

// ------------------------------------------------------------------------------------------------
// K0: per-column pre-pass
// ------------------------------------------------------------------------------------------------
// Three shapes of the pre-pass kernel, the same code: 1 024 threads x 4 (or 8) elements each (16 waves: the fastest way
// through ONE column, and what the library runs on single-round launches), 256 threads x 16 elements (4 waves, one per SIMD, 96 VGPRs: a
// workgroup that fits a CU as soon as ONE workgroup of a running pair kernel retires, where the 1 024-thread shape needs
// all four SIMDs' registers, i.e. an EMPTY CU).  The small shape was built in round 4 to let the later chunks of the
// pipelined host path sort beside the pair kernel; measured, that overlap makes the call longer (both kernels are bound
// by vector issue; icikt_capi.cpp, upload_and_prepare), so it is kept as an option of the debug plan (k0=1) and a test.
// A third shape, 512 threads x 8 elements (8 waves, 128 VGPRs, no spills): TWO workgroups -- two columns -- fit a CU (16
// waves, the register file, 2 x 74.5 KB of its 160 KB of LDS), so one column's dependent passes (each waits on a global
// round trip) run under the other's.  That pays when the launch has more columns than the device has CUs; a launch of
// one round is fastest with the 1 024-thread workgroup.  The host picks (icikt_k0plan.h: k0_pick_shape; plan key k0=2).
// Static LDS per workgroup as the compiler lays it out (bitsets for the longest column, 65 535 rows; per-wave scratch by
// the shape's waves; a sort area of 1.5 tiles): large 76 576 B, large8 125 728 B, small 76 192 B, pair 76 320 B, wide 66 080 B.
constexpr int K0_THREADS = 1024;   // the large shape
constexpr int K0_THREADS_SMALL = 256;
constexpr int K0_THREADS_PAIR = 512;
constexpr int K0_WORDS = 1024;     // words of a bitset over the rows of the longest column the tuned shapes take (65 535)
constexpr int K0_LDS_PAIR_MAX = 80 * 1024;   // what a workgroup of the pair shape may use: half a CU's LDS
#ifndef ICIKT_K0_MIN_WAVES
#define ICIKT_K0_MIN_WAVES 4   // waves per SIMD the pre-pass is compiled for: 4 = one 1 024-thread workgroup per CU (<= 128 VGPRs)
#endif
#ifndef ICIKT_K0_WAVES_SMALL
#define ICIKT_K0_WAVES_SMALL 5    // the small shape is compiled for five waves per SIMD (<= 96 registers): a wave of it fits a SIMD on which ONE pair-kernel wave (80 of 512 registers, six resident) has retired
#endif
constexpr int K0_UB = 8;       // iterations of a column pass whose loads a thread issues together
#ifdef ICIKT_K0_NO_NETWORK   // diagnostic build: keys built, stored and read back, no compare-exchange runs -- what the
constexpr bool K0_NETWORK = false;   // pre-pass takes without its sort (tools/k0_time.py --no-network); its results are WRONG
#else
constexpr bool K0_NETWORK = true;
#endif
constexpr int K0_TILE = 4096;  // elements of the LDS-resident sort tile (48 KB) = threads x elements per thread of the standard shapes

__device__ __forceinline__ unsigned long long sortable_key(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 and +0.0 tie (x[i] < x[j] is false both ways, kendallc.cpp:9,23)
  long long b = __double_as_longlong(v);
  unsigned long long u = (unsigned long long)b;
  return (b < 0) ? ~u : (u | 0x8000000000000000ull);
}

// ---- bitonic stages held in registers ---------------------------------------------------------------
// Thread t owns the E consecutive elements E t .. E t + E - 1 of the tile (E = 4 with 1 024 threads, 16 with 256):
// compare-exchange distances below E stay inside the thread, distances E .. 32 E pair it with lane t ^ (j / E) of its own
// wave (DPP and permlane exchanges: no LDS, no barrier); only distances >= 64 E need the LDS tile and a workgroup barrier.
// FAST: the element is ONE word, top 48 bits of the sortable key | row (16 bits) -- unique, so a single 64-bit compare
// orders it and no index travels beside it: five vector instructions per element of a lane stage instead of nine, two
// registers instead of three, 8 bytes per element through the LDS tile and the scratch instead of 12.  Exact whenever no
// two values of the column differ ONLY in the low 16 bits of their keys (relative difference below 2^-36): k0_prepare
// checks the result against the full keys and repeats the column with the three-word elements if it finds an inversion.
template <bool FAST>
__device__ __forceinline__ bool kv_gt(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib) {
  if constexpr (FAST) return ka > kb;
  return (ka > kb) || (ka == kb && ia > ib);
}
// stages j = jmax .. 1 (jmax <= 32 E) of merge step k; gi = global index of the thread's first element
template <bool FAST, int E>
__device__ __forceinline__ void k0_reg_stages(unsigned long long (&ek)[E], uint32_t (&ei)[E], int k, int jmax,
                                              int gi, int tid) {
  const uint32_t lane = (uint32_t)tid & 63u;
  const bool upw = (gi & k) == 0;  // lane stages run for k >= 2 E: the direction is the same for the thread's elements
  // one stage: partner lane = lane ^ LX (element distance E * LX), exchanged in registers (lane_xor: DPP / permlane)
#define ICIKT_K0_XSTAGE(LX)                                                                              \
  if (jmax >= E * (LX)) {                                                                                \
    const bool want_gt = (((tid & (LX)) == 0) == upw); /* take the partner's when (mine > theirs) == want_gt */ \
    _Pragma("unroll") for (int r = 0; r < E; ++r) {                                                      \
      const uint32_t klo = lane_xor<(LX)>((uint32_t)ek[r], lane), khi = lane_xor<(LX)>((uint32_t)(ek[r] >> 32), lane); \
      const uint32_t oi = FAST ? 0u : lane_xor<(LX)>(ei[r], lane);                                       \
      const unsigned long long ok = (unsigned long long)klo | ((unsigned long long)khi << 32);           \
      if (kv_gt<FAST>(ek[r], ei[r], ok, oi) == want_gt) { ek[r] = ok; ei[r] = oi; }                      \
    }                                                                                                    \
  }
  ICIKT_K0_XSTAGE(32) ICIKT_K0_XSTAGE(16) ICIKT_K0_XSTAGE(8) ICIKT_K0_XSTAGE(4) ICIKT_K0_XSTAGE(2) ICIKT_K0_XSTAGE(1)
#undef ICIKT_K0_XSTAGE
  // inside the thread: distances E / 2 .. 1; the direction of a pair follows its lower element (bit k of gi + a: for
  // k >= E that of gi, below it the bit of a itself)
#pragma unroll
  for (int j = E / 2; j >= 1; j >>= 1) {
    if (jmax >= j) {
#pragma unroll
      for (int a = 0; a < E; ++a) {
        if ((a & j) == 0) {
          const int b = a | j;
          const bool up = ((gi + a) & k) == 0;
          if (kv_gt<FAST>(ek[a], ei[a], ek[b], ei[b]) == up) {
            const unsigned long long tk = ek[a]; ek[a] = ek[b]; ek[b] = tk;
            const uint32_t ti = ei[a]; ei[a] = ei[b]; ei[b] = ti;
          }
        }
      }
    }
  }
}

// Compare-exchange stages on an array (the LDS tile, or the column's global scratch), TWO stages per pass and barrier: a
// thread loads the four elements i0, i0 + j/2, i0 + j, i0 + 3j/2, runs stage j (pairs at distance j) and stage j/2 in
// registers and stores them back -- half the barriers and half the traffic of one stage per pass.  Stages jmax .. jmin
// (powers of two) of merge step k over `count` elements; dbase = what is added to an index to find its direction bit.
template <bool FAST, int NT, typename KP, typename IP>
__device__ __forceinline__ void k0_mem_stages(KP tk, IP ti, int count, int dbase, int k, int jmax, int jmin, int tid) {
  int j = jmax;
  while (j >= 2 * jmin) {
    const int jh = j >> 1;
    for (int t = tid; t < (count >> 2); t += NT) {
      const int i0 = ((t & ~(jh - 1)) << 2) | (t & (jh - 1));
      const bool up = ((dbase + i0) & k) == 0;      // the same for the four: bits j/2 and j of i0 are clear, j + j/2 < k
      unsigned long long ek[4];
      uint32_t ei[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { ek[r] = tk[i0 + r * jh]; ei[r] = FAST ? 0u : ti[i0 + r * jh]; }
#define ICIKT_CE4(a, b)                                                              \
      if (kv_gt<FAST>(ek[a], ei[a], ek[b], ei[b]) == up) {                           \
        const unsigned long long xk = ek[a]; ek[a] = ek[b]; ek[b] = xk;              \
        const uint32_t xi = ei[a]; ei[a] = ei[b]; ei[b] = xi;                        \
      }
      ICIKT_CE4(0, 2) ICIKT_CE4(1, 3) ICIKT_CE4(0, 1) ICIKT_CE4(2, 3)
#undef ICIKT_CE4
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        tk[i0 + r * jh] = ek[r];
        if (!FAST) ti[i0 + r * jh] = ei[r];
      }
    }
    __syncthreads();
    j >>= 2;
  }
  if (j >= jmin) {   // an odd number of stages: the last one alone
    for (int t = tid; t < (count >> 1); t += NT) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      const int l = i | j;
      const bool up = ((dbase + i) & k) == 0;
      const unsigned long long ka = tk[i], kb = tk[l];
      const uint32_t ia = FAST ? 0u : ti[i], ib = FAST ? 0u : ti[l];
      if (kv_gt<FAST>(ka, ia, kb, ib) == up) {
        tk[i] = kb; tk[l] = ka;
        if (!FAST) { ti[i] = ib; ti[l] = ia; }
      }
    }
    __syncthreads();
  }
}

// ---- the tie program of a column (PrepView::tprog, srow, smask) ---------------------------------------------------
// From where a column's tie groups begin, the half-wave pair kernels walk it in steps cut at group boundaries:
//   HOT    64 singleton rows;
//   MIXED  two SUB-STEPS of up to 32 rows each, every one made of COMPLETE groups of at most 32 rows: no group
//          straddles the two, so rows of one group only ever meet inside a sub-step, in registers;
//   SOLO   a MIXED step whose sub-steps hold ONE group each (k0_step_at);
//   GROUP  up to 64 rows of ONE longer group (`closes`: the step holds the group's last row).
// The cut depends on the streamed column alone, so it is made here, once per column, by one wave (the step sequence is
// scalar code: every lane computes the same values, lane 0 stores) instead of by every pair that streams the column --
// S - 1 times, on the scalar unit of the pair kernel, with the flag words fetched from memory inside its step loop.
// Every step gets its RECORD (PrepView::srow): its rows in the lane layout the pair kernel runs it in, the guard row in
// the empty lanes.  For a MIXED / SOLO step the record also says, per lane, WHICH FLAGS of the pair kernel's in-step compare
// vectors (half_step_flags: bit layout below) belong to pairs inside a tie group (PrepView::smask: the masks of the lane's
// two rows, one per sub-step, combined): the pair kernel masks them out of the discordance count and counts the joint
// ties among them, whatever the sizes of the groups.
// gf: the column's group-start flags in PROCESSING order, W words + a zero guard word (in LDS).  The program starts at
// pos0 = 64 floor(hot_until / 64), where the pair kernel's singleton loop ends, and runs to n.
//
// Flag layout of half_step_flags (lane = (pair h, l = 0..31), DPP row = l >> 4, p = l & 15; sub-step s of the lane's two
// rows in byte s ("b" slots) and byte 2 + s ("a" slots) of both vectors):
//   vector 1   a bit i = in-row distance 2i + 1, b bit i = in-row distance 2i + 2 (i <= 6); b bit 7 = rows crossed at
//              rotation 0.  In-row distance d: the lane is the LATER row, its partner sits d lanes in front.
//   vector 2   a bit 4 + i = rotation 2i + 1, b bit 4 + i = rotation 2i + 2 (i <= 2); rotation 7 = bit 15 (s = 0) / 31.
//   rotation r of an UPPER-row lane: the lane is the later row, its partner the lower row's lane (p - r) mod 16, i.e.
//   D = (p >= r ? 16 + r : r) lanes in front; of a LOWER-row lane: the lane is the EARLIER row, its partner the upper
//   row's lane (p - r - 1) mod 16, D = (p - r - 1 >= 0 ? 15 - r : 31 - r) lanes behind.
// Two rows D lanes apart belong to one group iff D <= idx of the later one (rows of its group in front of it) iff
// D <= fwd of the earlier one (rows of its group behind it).
// The cross-row part of a row's masks depends on its lane and on ONE number, lim = idx of an upper-row lane / fwd of a
// lower-row lane (<= 31): a table [32][64] in LDS, filled once per workgroup, replaces eight compares per row and step.
//   bit 7: vector 1, rotation 0; bits 4..6: vector 2, rotations 2 4 6 (b slots); bits 12..14: rotations 1 3 5 (a slots);
//   bit 16: rotation 7
__device__ inline void k0_cross_table(uint32_t* T, int tid, int nthreads) {
  for (int i = tid; i < 32 * 64; i += nthreads) {
    const uint32_t lim = (uint32_t)i >> 6, l = (uint32_t)i & 31u, p = l & 15u;
    const bool upper = (l & 16u) != 0u;
    uint32_t t = 0u;
    for (uint32_t r = 0; r < 8; ++r) {
      const uint32_t D = upper ? ((p >= r) ? 16u + r : r) : ((p >= r + 1u) ? 15u - r : 31u - r);
      if (D > lim) continue;
      if (r == 0u) t |= 0x80u;
      else if (r == 7u) t |= 0x10000u;
      else if (r & 1u) t |= 0x1000u << ((r - 1u) >> 1);
      else t |= 0x10u << ((r - 2u) >> 1);
    }
    T[i] = t;
  }
}

// One step's entry, as if a step STARTED at position pos (every position is evaluated, in parallel; the steps the walk
// really takes are then picked out by following the chain).  16 bits: the layout of PrepView::tprog entries.
__device__ __forceinline__ uint32_t k0_step_at(const unsigned long long* gf, int n, int W, int pos) {
  const int wc = pos >> 6, fb = pos & 63;
  const unsigned long long w0 = gf[min(wc, W)], w1 = gf[min(wc + 1, W)];
  unsigned long long F = fb ? ((w0 >> fb) | (w1 << (64 - fb))) : w0;
  const bool fnbit = ((w1 >> fb) & 1ull) != 0ull;          // position pos + 64 starts a group
  const int remaining = n - pos;
  if (remaining < 64) F &= (1ull << remaining) - 1ull;
  const int avail = (remaining <= 64) ? remaining : 64;
  const bool endbit = fnbit || remaining == 64;            // offset 64 starts a group / is the end of the data
  if (avail == 64 && F == ~0ull && endbit) return 64u | (TPROG_KIND_HOT << 7) | (1u << 9);
  // group boundaries of the window: the starts, and the end of the data (one marker: no boundary beyond it)
  const unsigned long long Fe = (avail < 64) ? (F | (1ull << avail)) : F;
  const unsigned long long Fr = Fe & ~1ull;
  const int next = (Fr != 0ull) ? (int)__builtin_ctzll(Fr) : (endbit ? 64 : 65);   // end of the group at pos
  if ((F & 1ull) == 0ull || next > TPROG_KS) {
    const int glim = min(remaining, 64);
    return (uint32_t)min(next, glim) | (TPROG_KIND_GROUP << 7) | ((next <= glim) ? (1u << 9) : 0u);
  }
  // MIXED.  Sub-step 0: up to the last boundary within 32 rows (there is one: the first group has at most 32 rows);
  // sub-step 1: from b0 up to the last boundary within the next 32 rows -- none: the next group is longer (or the
  // data end at b0) and the step ends at b0.  The boundary at offset 64 (b0 == 32 only) is `endbit`.
  const int b0 = 63 - (int)__builtin_clzll(Fe & 0x1FFFFFFFEull);
  unsigned long long rest = (Fe >> b0) & 0x1FFFFFFFEull;
  if (b0 == 32 && endbit) rest |= 1ull << 32;
  const int b1 = (rest != 0ull) ? (63 - (int)__builtin_clzll(rest)) : 0;
  // SOLO: a MIXED step whose sub-steps hold ONE group each (sub-step 0 = the group at pos, sub-step 1 = the next group or
  // nothing): no pair of its rows is discordant inside a sub-step, so a pair kernel whose gathered columns have counter
  // tables runs it without the in-step chains (k1_pairs: hot_step<2>); otherwise it is a MIXED step like any other.
  const bool one0 = next == b0;
  const unsigned long long in1 = (Fe >> b0) & ((b1 > 1) ? ((1ull << b1) - 2ull) : 0ull);   // starts strictly inside sub-step 1
  const bool solo = one0 && in1 == 0ull;
  return (uint32_t)(b0 + b1) | ((solo ? TPROG_KIND_SOLO : TPROG_KIND_MIXED) << 7) | (1u << 9) | ((uint32_t)b0 << 10);
}

// the same-group flag masks of the rows of the MIXED step that starts at pos (entry e): one lane per row
// (returns the class of the step's largest group, wave-uniform: half_step_flags_near)
__device__ __forceinline__ uint32_t k0_step_masks(const unsigned long long* gf, const uint32_t* crossT, int n, int W, int pos,
                                                  uint32_t e, uint2& m_out, uint32_t lane) {
  const uint32_t b0 = tprog_n0(e), b1 = tprog_rows(e) - b0;
  const uint32_t sb = lane >> 5, l = lane & 31u;
  const bool vrow = l < (sb ? b1 : b0);          // (every lane of the wave stays: the step's largest group is a wave maximum)
  const int wc = pos >> 6, fb = pos & 63;
  const unsigned long long w0 = gf[min(wc, W)], w1 = gf[min(wc + 1, W)];
  unsigned long long Fe = fb ? ((w0 >> fb) | (w1 << (64 - fb))) : w0;
  const int remaining = n - pos;
  if (remaining < 64) Fe = (Fe & ((1ull << remaining) - 1ull)) | (1ull << remaining);
  const uint32_t o = min(sb ? b0 + l : l, 63u);                                   // offset of the row in the window (< 64)
  const unsigned long long upto = Fe & ((o < 63u) ? ((2ull << o) - 1ull) : ~0ull);
  const uint32_t idx = o - (63u - (uint32_t)__builtin_clzll(upto | 1ull));        // bit 0 is set: the step starts a group
  const unsigned long long above = (o < 63u) ? (Fe >> (o + 1u)) : 0ull;
  const uint32_t nxt = (above != 0ull) ? (o + 1u + (uint32_t)__builtin_ctzll(above)) : 64u;   // (offset 64: the step ends there)
  const uint32_t fwd = nxt - 1u - o;
  // class of the step's largest group: which distances of the pair kernel's second flag chain can hold a pair of one group
  const int gmax = __builtin_amdgcn_readfirstlane(wave_max_i32(vrow ? (int)(idx + fwd + 1u) : 0));
  const uint32_t cls = (gmax <= 3) ? 0u : (gmax <= 5) ? 1u : (gmax <= 9) ? 2u : 3u;
  m_out = make_uint2(0u, 0u);
  if (!vrow) return cls;
  const uint32_t p = l & 15u;
  const uint32_t c = min(min(idx, p), 15u);                                       // in-row partners inside my group
  const uint32_t a1 = (1u << ((c + 1u) >> 1)) - 1u, b1m = (1u << (c >> 1)) - 1u;   // vector 1: a / b slots
  const uint32_t t = crossT[min((l & 16u) ? idx : fwd, 31u) * 64u + lane];
  const uint32_t sh = 8u * sb;
  uint2 m;
  m.x = ((b1m | (t & 0x80u)) << sh) | (a1 << (16u + sh));
  m.y = ((t & 0x70u) << sh) | (((t >> 8) & 0x70u) << (16u + sh)) | ((t & 0x10000u) ? (0x8000u << (16u * sb)) : 0u);
  m_out = m;
  return cls;
}

// The whole workgroup builds the program, a WINDOW of TPROG_WIN positions at a time: (A) every position's would-be step,
// in parallel, into E (u16 per position of the window, LDS); (B) one wave follows the chain from where it stands -- one
// LDS read per step instead of a hundred dependent scalar operations -- while the step STARTS inside the window, writes
// the entries and lists the steps; (C) the waves share out the window's steps and write their RECORDS (PrepView::srow,
// smask): the step's rows in the lane layout the pair kernel runs it in -- an empty lane names the guard row -- and, for
// a MIXED step, per lane l = 0..31 the same-group masks of its two rows (sub-step 0: lane l, sub-step 1: lane l + 32).
// Steps per window: a MIXED step that does not reach 33 rows is followed by a group of more than 32 rows, and a closing
// GROUP step that does not reach 33 rows follows a 64-row piece of its group: any two consecutive steps hold >= 34 rows
// -- at most TPROG_WIN / 17 + 1 steps start in a window, n / 17 + 2 in a column (PrepView::sr_steps has room for them and
// for the three guard steps behind the last one: what the pair kernel loads ahead).
// scratch: E (TPROG_WIN u16) | list of the window's steps (TPROG_LIST pairs of u16: window offset, entry index) | crossT
// (32 x 64 u32); `cnt`: four shared ints (steps of the window; the chain's position and entry count between windows; the
// column's streaming cost, see below).
// SEGMENT MARKS (round 4, last change): four positions of the walk at which a pair kernel task may be CUT when a launch has
// fewer tasks than the chip has waves -- the wave that takes the part behind a mark first inserts the rows in front of it
// without counting them (k1_pairs).  A mark is the start of a step that starts a tie group (or a multiple of 64 inside the
// singleton region); marks 1 cuts the walk in two parts of equal cost, marks 0, 2, 3 in four (inserting a row costs about
// an eighth of counting it; the closed-form tail costs next to nothing).  Written behind the program: prog_tail[0..3] =
// positions (0xFFFFFFFF: none), prog_tail[4..7] = their program steps (0xFFFFFFFF: in the singleton region).
__device__ inline void k0_tie_program(const unsigned long long* gf, uint16_t* E, uint16_t* mlist, uint32_t* crossT, int* cnt,
                                      int n, int W, uint32_t* prog, uint32_t* prog_tail, const uint16_t* ord, uint16_t* srow,
                                      uint2* smask, int sr_steps, uint32_t guard_row, int tid, int nthreads) {
  const uint32_t lane = (uint32_t)tid & 63u;
  const int wave = tid >> 6, nwaves = nthreads >> 6;
  k0_cross_table(crossT, tid, nthreads);
  if (wave == 0) {
    int first_cont = n, best = 0;   // first position that continues a group; highest group start
    for (int w = (int)lane; w < W; w += 64) {
      unsigned long long f = gf[w], z = ~gf[w];
      if (w == W - 1 && (n & 63)) { f &= (1ull << (n & 63)) - 1ull; z &= (1ull << (n & 63)) - 1ull; }
      if (z != 0ull) first_cont = min(first_cont, w * 64 + (int)__builtin_ctzll(z));
      if (f != 0ull) best = max(best, w * 64 + 63 - (int)__builtin_clzll(f));
    }
    first_cont = -__builtin_amdgcn_readfirstlane(wave_max_i32(-first_cont));
    const int last_start = __builtin_amdgcn_readfirstlane(wave_max_i32(best));
    const int hot_until = (first_cont < n) ? first_cont - 1 : n;
    const int pos0 = (hot_until >> 6) << 6;
    // cnt[3]: what streaming this column costs a pair, in half hot steps (a hot step of 64 rows = 2, a MIXED step = 3, a
    // GROUP step = 3: their vector instructions): the singleton region now, the program's steps below
    if (lane == 0u) {
      cnt[1] = pos0; cnt[2] = 0; cnt[3] = 2 * (hot_until >> 6);
      // the segment marks: targets as shares of the rows in front of the last tie group (it runs in closed form when it is
      // longer than a step); those inside the singleton region are known now, the others are met by the walk below
      const int n_eff = (n - last_start > 64) ? last_start : n;
      const int share[TPROG_MARKS] = {307, 545, 578, 815};   // (in 1 / 1024: 0.300, 0.532, 0.564, 0.796 of the rows)
      for (int j = 0; j < TPROG_MARKS; ++j) {
        const int T = (int)(((uint32_t)n_eff * (uint32_t)share[j]) >> 10);   // (n <= 65 535: fits 32 bits)
        cnt[12 + j] = T;
        if (T < pos0) { cnt[4 + j] = (T >> 6) << 6; cnt[8 + j] = -1; }   // (step -1: in the singleton region)
        else { cnt[4 + j] = -1; cnt[8 + j] = -1; }                         // (position -1: not met yet)
      }
      cnt[16] = 0;   // the walk stands inside a group of several GROUP steps
    }
  }
  __syncthreads();
  for (int win = (cnt[1] / TPROG_WIN) * TPROG_WIN; win < n; win += TPROG_WIN) {
    const int wend = min(n, win + TPROG_WIN);
    for (int p = win + tid; p < wend; p += nthreads) E[p - win] = (uint16_t)k0_step_at(gf, n, W, p);
    __syncthreads();
    if (wave == 0) {
      int pos = cnt[1], ne = cnt[2], ns = 0, cost = cnt[3];
      int mpos[TPROG_MARKS], mstep[TPROG_MARKS], mT[TPROG_MARKS];
      for (int j = 0; j < TPROG_MARKS; ++j) { mpos[j] = cnt[4 + j]; mstep[j] = cnt[8 + j]; mT[j] = cnt[12 + j]; }
      bool open = cnt[16] != 0;
      int mj = 0;   // marks met so far (those inside the singleton region were set before the walk)
      while (mj < TPROG_MARKS && mpos[mj] >= 0) ++mj;
      int nextT = (mj < TPROG_MARKS) ? mT[mj] : 0x7FFFFFFF;   // the next mark's target: one compare per step of the walk
      while (pos < wend) {
        const uint32_t e = (uint32_t)E[pos - win];
        // (the targets ascend: the marks are met in turn, one compare per step)
        if (!open && pos >= nextT) {   // (rare: four times per column)
          while (mj < TPROG_MARKS && pos >= mT[mj]) { mpos[mj] = pos; mstep[mj] = ne; ++mj; }
          nextT = (mj < TPROG_MARKS) ? mT[mj] : 0x7FFFFFFF;
        }
        open = tprog_kind(e) == TPROG_KIND_GROUP && !tprog_closes(e);
        cost += (tprog_kind(e) == TPROG_KIND_HOT) ? 2 : 3;
        if (lane == 0u) {
          prog[ne] = e;
          if (ns < TPROG_LIST) { mlist[2 * ns] = (uint16_t)(pos - win); mlist[2 * ns + 1] = (uint16_t)ne; }
        }
        ++ns;
        ++ne;
        pos += (int)tprog_rows(e);
      }
      if (lane == 0u) {
        if (wend == n) prog[ne] = 0u;
        cnt[0] = min(ns, TPROG_LIST); cnt[1] = pos; cnt[2] = ne; cnt[3] = cost;
        for (int j = 0; j < TPROG_MARKS; ++j) { cnt[4 + j] = mpos[j]; cnt[8 + j] = mstep[j]; }
        cnt[16] = open ? 1 : 0;
      }
    }
    __syncthreads();
    const int ns = cnt[0];
    for (int i = wave; i < ns; i += nwaves) {
      const int pos = win + (int)mlist[2 * i];
      const int st = (int)mlist[2 * i + 1];
      if (st + 3 >= sr_steps) continue;   // (cannot happen: the bound above)
      const uint32_t e = (uint32_t)E[pos - win];
      const uint32_t rows = tprog_rows(e);
      if (tprog_kind(e) == TPROG_KIND_MIXED || tprog_kind(e) == TPROG_KIND_SOLO) {
        const uint32_t b0 = tprog_n0(e), sb = lane >> 5, l = lane & 31u;
        const bool vrow = l < (sb ? rows - b0 : b0);
        srow[st * 64 + (int)lane] = (uint16_t)(vrow ? (uint32_t)ord[(uint32_t)pos + (sb ? b0 + l : l)] : guard_row);
        uint2 m;
        const uint32_t cls = k0_step_masks(gf, crossT, n, W, pos, e, m, lane);
        m.x |= (uint32_t)__shfl_xor((int)m.x, 32, 64);
        m.y |= (uint32_t)__shfl_xor((int)m.y, 32, 64);
        if (lane < 32u) smask[st * 32 + (int)lane] = m;
        // the class of the step's largest group rides in the step's entry (bits 16..17), which the pair kernel holds two
        // steps ahead; the entry was written by wave 0 before the barrier above
        if (lane == 0u && cls != 0u) prog[st] |= cls << 16;
      } else {
        srow[st * 64 + (int)lane] = (uint16_t)((lane < rows) ? (uint32_t)ord[(uint32_t)pos + lane] : guard_row);
      }
    }
    __syncthreads();   // (E and the list are rewritten by the next window)
  }
  // three guard steps behind the last one (the pair kernel reads its rows three steps ahead)
  {
    const int ne = cnt[2];
    if (ne + 3 <= sr_steps)
      for (int i = tid; i < 192; i += nthreads) srow[ne * 64 + i] = (uint16_t)guard_row;
  }
  if (tid < 2 * TPROG_MARKS) prog_tail[tid] = (uint32_t)cnt[4 + tid];   // (-1 -> 0xFFFFFFFF)
}

// WIDE (65 535 < n): 32-bit positions in separate arrays (order32, q32, lo32, hi32), the phase-3 bitsets in global
// memory (they outgrow the static LDS), no tie-group list and no rec staging.
template <bool WIDE, int NT, int E>
__device__ __forceinline__ void k0_prepare_body(const PrepView& pv, const double* __restrict__ X, int64_t ld, int col_begin,
                                                const MaskSpec& ms, uint8_t* __restrict__ keep) {
  static_assert((NT == K0_THREADS || NT == K0_THREADS_SMALL || NT == K0_THREADS_PAIR) && (E == 4 || E == 8 || E == 16), "pre-pass shapes");
  constexpr int TILE = NT * E;                      // elements of the LDS-resident sort tile
  constexpr int NW = NT / 64;                       // waves of the workgroup
  constexpr int NI = (8 * NW > 32) ? 8 * NW : 32;   // ints of scratch: eight per wave (the statistics), the tie program's 17
  static_assert(3 * NW <= K0_WORDS && TPROG_WIN * 2 + 2048 * 4 + TPROG_LIST * 4 <= (TILE + TILE / 2) * 8, "pre-pass scratch");
  __shared__ long long sh_ll[K0_WORDS];             // phase 3: the bitset of the groups of >= 2 rows; three words per wave at the end
  __shared__ int sh_i[NI];
  __shared__ unsigned long long sh_bits_lds[K0_WORDS];  // fill-group bitset, W <= 1024 words
  __shared__ unsigned long long sh_st_lds[K0_WORDS + 4];    // phase 1: the min reduction; phase 3: group starts, n + 1 <= 65 536 bits
  unsigned long long* const sh_bits = WIDE ? pv.k0_bits + (size_t)blockIdx.x * 2 * (size_t)(pv.Wp + 1) : sh_bits_lds;
  unsigned long long* const sh_st = WIDE ? sh_bits + (pv.Wp + 1) : sh_st_lds;
  __shared__ unsigned long long sh_sort[TILE + TILE / 2];  // 48 KB (96 KB: E = 8 with 1 024 threads): the sort tile, later the rec staging area
  __shared__ uint16_t sh_bigpre[K0_WORDS];          // phase 3: tie groups of >= 2 rows that start in the words before w
  static_assert(NT != K0_THREADS_PAIR ||
                sizeof(sh_ll) + sizeof(sh_i) + sizeof(sh_bits_lds) + sizeof(sh_st_lds) + sizeof(sh_sort) + sizeof(sh_bigpre) <= (size_t)K0_LDS_PAIR_MAX,
                "two workgroups of the pair shape share a CU's 160 KB of LDS");
  unsigned long long* sh_tk = sh_sort;                                      // sort tile: keys
  uint32_t* sh_ti = reinterpret_cast<uint32_t*>(sh_sort + TILE);         // sort tile: row indices
  uint32_t* rec_s = reinterpret_cast<uint32_t*>(sh_sort);                   // after the sort: rec by row
  // The per-row arrays are written by ROW (scattered): through the free sort tile, then out in order, as far as it holds
  // them -- rec and (hi | tie-group index << 16) for columns of up to 3 TILE / 2 rows (12 288 with the 8 192-element tile),
  // the latter alone (two scattered 2-byte stores per row otherwise, against one 4-byte store for rec) up to 3 TILE rows
  const bool stage_hg = !WIDE && pv.n_pad <= 3 * TILE;
  const bool stage_rec = stage_hg && 2 * pv.n_pad <= 3 * TILE;
  uint32_t* hg_s = stage_rec ? rec_s + pv.n_pad : rec_s;
  // girow: every column the half-wave pair kernels can run on; longer columns when they hold more than K1_CNT_MIN_GROUPS tie
  // groups (the whole-wave kernels' count mode asks for nothing less: decided per column below, once its groups are counted)
  bool want_gi = pv.tp_stride > 0;

  const int c = col_begin + blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int n = pv.n;
  const int W = pv.W;
  const int npow2 = pv.npow2;
  const double* col = X + (int64_t)c * ld;
  unsigned long long* keys = pv.sort_keys + (int64_t)blockIdx.x * npow2;
  uint32_t* idx = pv.sort_idx + (int64_t)blockIdx.x * npow2;
  unsigned long long* mask = pv.col_mask(c);
  unsigned long long* fmask = pv.col_fillmask(c);
  unsigned long long* gflag = pv.col_gflag(c);
  uint16_t* order = WIDE ? nullptr : pv.order + (int64_t)c * pv.n_ord;
  uint32_t* rec = WIDE ? nullptr : pv.rec + ((int64_t)(c >> 1) * pv.rec_rows) * 2 + (c & 1);  // [block][row][2]: stride 2
  uint16_t* hirow = WIDE ? nullptr : pv.hirow + ((int64_t)(c >> 1) * pv.rec_rows) * 2 + (c & 1);            // [block][row][2]: stride 2
  uint16_t* girow = WIDE ? nullptr : pv.girow + ((int64_t)(c >> 1) * pv.rec_rows) * 2 + (c & 1);            // likewise
  if (!WIDE && tid == 0) {   // the guard row (PrepView::rec_rows)
    rec[2 * pv.n_pad] = (uint32_t)pv.n_pad; hirow[2 * pv.n_pad] = 0; girow[2 * pv.n_pad] = GIROW_NONE;
  }
  uint32_t* tgl = WIDE ? nullptr : pv.tgroups + (int64_t)c * pv.tg_stride;
  uint32_t* order32 = WIDE ? pv.order32 + (int64_t)c * pv.n_pad : nullptr;
  uint32_t* q32 = WIDE ? pv.q32 + (int64_t)c * pv.n_pad : nullptr;
  uint32_t* lo32 = WIDE ? pv.lo32 + (int64_t)c * pv.n_pad : nullptr;
  uint32_t* hi32 = WIDE ? pv.hi32 + (int64_t)c * pv.n_pad : nullptr;

  // ---- phase 1: NA bitset, NA count, min of the non-missing values (kendallc.cpp:187-218) --------
  // The caller's global_na rule (setup_missing_matrix, R/utils.R:1-23) is applied HERE, while the column is read:
  // an excluded cell is missing (R/kendalltau.R:119-121), and so is every NaN (Rcpp is_na, kendallc.cpp:181).
  double tmin = __longlong_as_double(0x7FF0000000000000ll);  // +Inf
  int nna = 0, nexcl = 0;
  uint8_t* keep_c = keep ? keep + (int64_t)c * n : nullptr;
  // (The passes over the column are BLOCKED: a thread issues the loads of K0_UB iterations, then consumes them.  One
  //  workgroup per CU hides no latency by itself, and with a ballot in the loop body the compiler keeps one load in
  //  flight per thread: a pass then cost one memory round trip per iteration -- ten for 10 000 rows -- and the passes
  //  outside the sort were half of the kernel's time.)
  for (int base0 = 0; base0 < pv.n_pad; base0 += NT * K0_UB) {
    double vv[K0_UB];
#pragma unroll
    for (int u = 0; u < K0_UB; ++u) {
      const int i = base0 + u * NT + tid;
      vv[u] = (i < n) ? col[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < K0_UB; ++u) {
      if (base0 + u * NT < pv.n_pad) {   // (uniform over the workgroup: the ballot runs with every lane)
        const int i = base0 + u * NT + tid;
        const double v = vv[u];
        const bool excl = (i < n) && mask_excluded(ms, v);
        const bool isna = (i < n) && (excl || v != v);
        nexcl += excl ? 1 : 0;
        if (keep_c && i < n) keep_c[i] = excl ? 0 : 1;
        const unsigned long long b = __ballot(isna);
        if (lane == 0 && (i >> 6) < W) {
          mask[i >> 6] = b;
          if (!WIDE) sh_bits_lds[i >> 6] = b;   // (the one-word sort compacts the column by it)
        }
        if (i < n && !isna) tmin = (v < tmin) ? v : tmin;
        nna += isna ? 1 : 0;
      }
    }
  }
  if (tid == 0) { mask[W] = 0ull; }
  // plain double min (no NaN among candidates), the missing and the excluded rows: one batch, two barriers
  {
    tmin = wave_reduce(tmin, [](double a, double b) { return (b < a) ? b : a; });
    nna = wave_reduce(nna, [](int a, int b) { return a + b; });
    nexcl = wave_reduce(nexcl, [](int a, int b) { return a + b; });
    double* sh_d = reinterpret_cast<double*>(sh_st_lds);   // (the start-flag bitset of phase 3 lives here later)
    if (lane == 0) { sh_d[tid >> 6] = tmin; sh_i[tid >> 6] = nna; sh_i[NW + (tid >> 6)] = nexcl; }
    __syncthreads();
    tmin = sh_d[0]; nna = sh_i[0]; nexcl = sh_i[NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const double b = sh_d[w];
      tmin = (b < tmin) ? b : tmin;
      nna += sh_i[w];
      nexcl += sh_i[NW + w];
    }
    __syncthreads();
  }
  const double fill = tmin - 0.1;  // kendallc.cpp:214-215, double arithmetic

  // ---- phases 1b + 2: sortable keys, sort.  FAST: one word per element (top 48 key bits | row), see kv_gt ------
  // The one-word sort orders only the column's PRESENT values, where that makes the network smaller.  A missing or excluded
  // row's key is `fill`, below every present value: the fill group is exactly those rows, in row order, so a row's place
  // in it is the number of set bits of the phase-1 bitset below it.  cna = rows kept out of the sort; 0 -- the column is
  // sorted whole, as the three-word sort always is -- when fill is not below the minimum (it rounds to it for
  // |min| > 2^49, and every row may be missing) or when the present values alone would take the same slots (c2-like
  // columns: the prefix counts and the second list would only cost).  sh_bigpre[w] = missing rows in the words before w
  // (phase 3 rewrites it).
  // What enters the network for x values (F = x / TILE full tiles, r = x mod TILE left over):
  //   np2   elements the tile sorts and merge levels run over, the first nreal of them real;
  //   m     a SUB-TILE behind them: the r left-over values, padded to a power of two (>= one wave's 64 E elements), sorted by
  //         the waves that hold them at offset sub_lo of the tile slot at np2.  F = 0: the whole sort, ascending.  F a power of
  //         two: the np2 = F TILE values in front are sorted without any padding and the sub-tile, descending at the END of
  //         its slot, is where a full sort of the upper half would have left its real elements; the last merge level then
  //         exchanges only the m pairs that reach it, merges the lower half as usual and the sub-tile with the distances
  //         below m (the stages above m would move it to the front of the upper half unchanged: it is stored there).
  //         The sorted values end up contiguous at keys[0 .. x).
  //   Other F (3, 5, 6, 7, ...): np2 = the power of two above x, tiles of padding skipped.
  //   Short columns (npow2 < TILE): the all-LDS sort at the size it has always had.
  // Returns the slots the network runs over.
  auto sort_plan = [&](int x, int& np2, int& nreal, int& m, int& sub_lo) -> int {
    np2 = npow2; nreal = x; m = 0; sub_lo = 0;
    if (npow2 < TILE) return np2;
    const int F = x / TILE, r = x - F * TILE;
    const int rp2 = (r <= 64 * E) ? 64 * E : (1 << (32 - __builtin_clz((uint32_t)(r - 1))));
    if (rp2 == TILE) np2 = 1 << (32 - __builtin_clz((uint32_t)(x - 1)));   // (more than half a tile left over: a tile like the others)
    else if (F == 0) { np2 = 0; nreal = 0; m = rp2; }
    else if ((F & (F - 1)) == 0 && r > 0) { np2 = nreal = F * TILE; m = rp2; sub_lo = K0_NETWORK ? TILE - m : 0; }
    else np2 = 1 << (32 - __builtin_clz((uint32_t)(x - 1)));   // (x >= TILE here)
    return np2 + m;
  };
  int cna = 0;
  if constexpr (!WIDE) {
    int a0, a1, a2, a3;
    if (nna > 0 && fill < tmin && sort_plan(n - nna, a0, a1, a2, a3) < sort_plan(n, a0, a1, a2, a3)) {   // (uniform over the workgroup)
      cna = nna;
      int pbase = 0;
      for (int wb = 0; wb < W; wb += NT) {
        const int wi = wb + tid;
        const int cnt = (wi < W) ? (int)__popcll(sh_bits_lds[wi]) : 0;
        const int incl = (int)wave_incl_scan((uint32_t)cnt);
        if (lane == 63) sh_i[tid >> 6] = incl;
        __syncthreads();
        int wbase = pbase, btot = 0;
        for (int w = 0; w < NW; ++w) {
          const int t = sh_i[w];
          if (w < (tid >> 6)) wbase += t;
          btot += t;
        }
        if (wi < W) sh_bigpre[wi] = (uint16_t)(wbase + incl - cnt);
        pbase += btot;
        __syncthreads();
      }
    }
  }

  auto sort_pass = [&](auto fast_tag) {
  constexpr bool FAST = decltype(fast_tag)::value;
  int np2 = npow2, nreal = n, m = 0, sub_lo = 0;
  if constexpr (FAST) {
    const int p = n - cna, r = p % TILE;
    sort_plan(p, np2, nreal, m, sub_lo);
    const int slot_end = ((m > 0) ? np2 + sub_lo + r : p);            // one past the last real element
    const int pad_end = (m > 0) ? np2 + sub_lo + m : np2;
    for (int base0 = 0; base0 < pv.n_pad; base0 += NT * K0_UB) {
      double vv[K0_UB];
#pragma unroll
      for (int u = 0; u < K0_UB; ++u) {
        const int i = base0 + u * NT + tid;
        vv[u] = (i < n) ? col[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < K0_UB; ++u) {
        const int i = base0 + u * NT + tid;
        if (i < n) {
          double v = vv[u];
          int q = 0;          // missing rows in front of row i
          bool gone = false;  // row i is one of them
          if (cna) {
            const unsigned long long w = sh_bits_lds[i >> 6];
            q = (int)sh_bigpre[i >> 6] + (int)__popcll(w & ((1ull << (i & 63)) - 1ull));
            gone = ((w >> (i & 63)) & 1ull) != 0ull;
          } else if (v != v || mask_excluded(ms, v)) {
            v = fill;
          }
          if (gone) {
            idx[q] = (uint32_t)i;   // its place in the ascending order
          } else {
            const int d = i - q;    // dense index among the present values
            keys[(d < np2 || m == 0) ? d : d + sub_lo] = (sortable_key(v) & ~0xFFFFull) | (unsigned long long)i;   // (n <= 65 535: the row fits the low 16 bits)
          }
        }
      }
    }
    for (int i = slot_end + tid; i < pad_end; i += NT) keys[i] = ~0ull;
  } else {
  for (int base0 = 0; base0 < npow2; base0 += NT * K0_UB) {
    double vv[K0_UB];
#pragma unroll
    for (int u = 0; u < K0_UB; ++u) {
      const int i = base0 + u * NT + tid;
      vv[u] = (i < n) ? col[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < K0_UB; ++u) {
      const int i = base0 + u * NT + tid;
      if (i < npow2) {
        unsigned long long k = ~0ull;
        uint32_t id = 0xFFFFFFFFu;
        if (i < n) {
          double v = vv[u];
          if (v != v || mask_excluded(ms, v)) v = fill;
          k = sortable_key(v);
          if (FAST) k = (k & ~0xFFFFull) | (unsigned long long)i;    // (n <= 65 535: the row fits the low 16 bits)
          id = (uint32_t)i;
        }
        keys[i] = k;
        if (!FAST) idx[i] = id;
      }
    }
  }
  }
  __syncthreads();

  // ---- phase 2: bitonic sort of (key, row): the row index breaks ties, which makes the result the
  //      stable order std::stable_sort gives in sortedIndex (kendallc.cpp:5-12).  Compare-exchange
  //      distances below the tile size run on an LDS-resident tile; only the long distances of the
  //      last merges touch global memory. -------------------------------------------------------------
  {
    const int T = (np2 < TILE && m == 0) ? np2 : TILE;
    const int ntiles = np2 / T;
    if (K0_NETWORK && T == TILE) {
      // full tiles: register / shuffle stages (k0_reg_stages) around the LDS stages with distance >= 256
      // (a wave holds 64 E consecutive elements: distances up to 32 E in registers, 64 E and more on the LDS tile)
      unsigned long long ek[E];
      uint32_t ei[E];
      for (int tile = 0; tile < ntiles; ++tile) {
        const int tb = tile * T;
        if (tb >= nreal) continue;  // a tile of padding only (equal keys) is sorted in either direction already
        const int gi = tb + E * tid;
#pragma unroll
        for (int r = 0; r < E; ++r) { ek[r] = keys[gi + r]; ei[r] = FAST ? 0u : idx[gi + r]; }
        for (int k = 2; k <= 64 * E; k <<= 1) k0_reg_stages<FAST, E>(ek, ei, k, k >> 1, gi, tid);
        for (int k = 128 * E; k <= T; k <<= 1) {
#pragma unroll
          for (int r = 0; r < E; ++r) { sh_tk[E * tid + r] = ek[r]; if (!FAST) sh_ti[E * tid + r] = ei[r]; }
          __syncthreads();
          k0_mem_stages<FAST, NT>(sh_tk, sh_ti, T, tb, k, k >> 1, 64 * E, tid);
#pragma unroll
          for (int r = 0; r < E; ++r) { ek[r] = sh_tk[E * tid + r]; ei[r] = FAST ? 0u : sh_ti[E * tid + r]; }
          __syncthreads();  // the tile is rewritten by the next step's stores
          k0_reg_stages<FAST, E>(ek, ei, k, 32 * E, gi, tid);
        }
#pragma unroll
        for (int r = 0; r < E; ++r) { keys[gi + r] = ek[r]; if (!FAST) idx[gi + r] = ei[r]; }
      }
      // the sub-tile (a body of its own: with run-time sizes in the loop above the full tiles' LDS passes lose their
      // compile-time trip counts): cnt elements at offset lo of the slot at np2, held by the waves `mine` (every thread stays
      // for the barriers); its last step sorts in the direction of bit kf of its index -- ascending in front of nothing (bit
      // T of slot 0), descending behind np2 values (bit np2 of the slot at np2)
      if constexpr (FAST) {
        if (m > 0) {
          const int tb = np2, lo = sub_lo, cnt = m, kf = (np2 > 0) ? np2 : T;
          const bool mine = E * tid >= lo && E * tid < lo + cnt;   // (whole waves: lo and cnt are multiples of 64 E)
          const int gi = tb + E * tid;
          if (mine) {
#pragma unroll
            for (int r = 0; r < E; ++r) { ek[r] = keys[gi + r]; ei[r] = 0u; }
            for (int k = 2; k <= 64 * E; k <<= 1) k0_reg_stages<FAST, E>(ek, ei, (k == cnt) ? kf : k, k >> 1, gi, tid);
          }
          for (int k = 128 * E; k <= cnt; k <<= 1) {
            const int kd = (k == cnt) ? kf : k;
            if (mine) {
#pragma unroll
              for (int r = 0; r < E; ++r) sh_tk[E * tid + r] = ek[r];
            }
            __syncthreads();
            k0_mem_stages<FAST, NT>(sh_tk + lo, sh_ti + lo, cnt, tb + lo, kd, k >> 1, 64 * E, tid);
            if (mine) {
#pragma unroll
              for (int r = 0; r < E; ++r) ek[r] = sh_tk[E * tid + r];
            }
            __syncthreads();
            if (mine) k0_reg_stages<FAST, E>(ek, ei, kd, 32 * E, gi, tid);
          }
          if (mine) {
#pragma unroll
            for (int r = 0; r < E; ++r) keys[gi + r] = ek[r];
          }
        }
      }
      __syncthreads();
      // merges across tiles: distances >= T in global memory, 2048..256 on the LDS tile, the rest in registers
      // With a sub-tile behind np2 values, one more level (k = 2 np2) merges the two: the upper half is padding but for the
      // sub-tile at its end, so of the level's first stage only the m pairs that reach the sub-tile can exchange; the lower
      // half then takes the level's other stages as usual, and the sub-tile those below m, as one more "tile" (ascending:
      // direction bit k of an index below T), stored at the front of the upper half.
      const int ktop = (m > 0 && np2 > 0) ? 2 * np2 : np2;
      for (int k = 2 * T; k <= ktop; k <<= 1) {
        const bool top = k > np2;
        if constexpr (FAST) {
          if (top) {
            for (int x = tid; x < m; x += NT) {
              const int i = np2 - m + x, l = np2 + sub_lo + x;
              const unsigned long long ka = keys[i], kb = keys[l];
              if (ka > kb) { keys[i] = kb; keys[l] = ka; }
            }
            __syncthreads();
          }
        }
        k0_mem_stages<FAST, NT>(keys, idx, np2, 0, k, top ? (np2 >> 1) : (k >> 1), T, tid);   // (global scratch: __syncthreads orders a workgroup's global accesses)
        for (int tile = 0; tile < ntiles + (top ? 1 : 0); ++tile) {
          const bool sub = tile == ntiles;
          const int tb = sub ? 0 : tile * T;                     // what the direction bit is taken from
          const int lo = sub ? sub_lo : 0, cnt = sub ? m : T;
          const bool mine = E * tid >= lo && E * tid < lo + cnt;
          const int src = tile * T + E * tid, gi = tb + E * tid;
          if (mine) {
#pragma unroll
            for (int r = 0; r < E; ++r) { sh_tk[E * tid + r] = keys[src + r]; if (!FAST) sh_ti[E * tid + r] = idx[src + r]; }
          }
          __syncthreads();
          // (the direction is constant inside a tile: k > T)
          if (sub) k0_mem_stages<FAST, NT>(sh_tk + lo, sh_ti + lo, cnt, tb, k, cnt >> 1, 64 * E, tid);
          else k0_mem_stages<FAST, NT>(sh_tk, sh_ti, TILE, tb, k, TILE >> 1, 64 * E, tid);
          if (mine) {
#pragma unroll
            for (int r = 0; r < E; ++r) { ek[r] = sh_tk[E * tid + r]; ei[r] = FAST ? 0u : sh_ti[E * tid + r]; }
          }
          __syncthreads();
          if (mine) {
            k0_reg_stages<FAST, E>(ek, ei, k, 32 * E, gi, tid);
#pragma unroll
            for (int r = 0; r < E; ++r) { keys[src - lo + r] = ek[r]; if (!FAST) idx[src - lo + r] = ei[r]; }
          }
        }
        __syncthreads();
      }
    } else {
      // short columns (npow2 < 4096): one partial tile, every stage on LDS
      for (int i = tid; i < T; i += NT) { sh_tk[i] = keys[i]; if (!FAST) sh_ti[i] = idx[i]; }
      __syncthreads();
      for (int k = 2; K0_NETWORK && k <= T; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = tid; t < (T >> 1); t += NT) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const int l = i | j;
            const bool up = ((i & k) == 0);
            const unsigned long long ka = sh_tk[i], kb = sh_tk[l];
            const uint32_t ia = FAST ? 0u : sh_ti[i], ib = FAST ? 0u : sh_ti[l];
            if (kv_gt<FAST>(ka, ia, kb, ib) == up) {
              sh_tk[i] = kb; sh_tk[l] = ka;
              if (!FAST) { sh_ti[i] = ib; sh_ti[l] = ia; }
            }
          }
          __syncthreads();
        }
      }
      for (int i = tid; i < T; i += NT) { keys[i] = sh_tk[i]; if (!FAST) idx[i] = sh_ti[i]; }
      __syncthreads();
    }
  }
  };   // sort_pass
  bool starts_done = false;   // the group-start bitset has been made (by the pass behind the one-word sort)
  if constexpr (WIDE) {
    sort_pass(std::false_type{});
  } else {
    // One-word elements first.  ONE pass then turns the sorted words into what phase 3 needs -- the row of every position
    // (idx) and the group-start bitset -- from the FULL keys (one gather of the column per position; a position's
    // predecessor is the lane below, a wave's first lane gathers its predecessor itself), and checks the order against the
    // full keys on the way: an inversion means two values of the column share the top 48 bits of their keys and differ
    // below them; the column is then sorted again with three-word elements (full key, row) and the bitset is made from
    // those.  Equal full keys are in row order either way: the row is part of the word.
    sort_pass(std::true_type{});
    // The sorted WORD decides most positions by itself: neighbours whose 48-bit prefixes differ are in order and start
    // a new group, and the cna rows in front (kept out of the sort, listed in idx) are one group, the fill group, below
    // every sorted value.  Only a position whose prefix equals a neighbour's gathers its full key -- its own, for its
    // successor's compare as much as for its own; a continuous column gathers nothing.
    int inv = 0;
    for (int base0 = 0; base0 <= ((n >> 6) << 6); base0 += NT * K0_UB) {
      // the sorted word, then -- where a prefix repeats -- the value of its row: issued K0_UB positions at a time
      unsigned long long wv[K0_UB], we[K0_UB];   // we: the word next to the wave (first lane: in front, last lane: behind)
      double vv[K0_UB], vp[K0_UB];
      bool samep[K0_UB], need[K0_UB];            // the prefix equals the predecessor's; the full key is wanted
#pragma unroll
      for (int u = 0; u < K0_UB; ++u) {
        const int k = base0 + u * NT + tid;
        const int ke = (lane == 0) ? k - 1 : k + 1;
        wv[u] = (k >= cna && k < n) ? keys[k - cna] : 0ull;
        we[u] = ((lane == 0 || lane == 63) && k >= cna && k < n && ke >= cna && ke < n) ? keys[ke - cna] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < K0_UB; ++u) {
        const int k = base0 + u * NT + tid;
        const unsigned long long p = wv[u] >> 16;
        unsigned long long pp = __shfl_up(p, 1, 64), pn = __shfl_down(p, 1, 64);
        if (lane == 0) pp = we[u] >> 16;
        if (lane == 63) pn = we[u] >> 16;
        const bool sorted = k >= cna && k < n;                  // the position holds a sorted word
        samep[u] = sorted && k > cna && pp == p;
        need[u] = samep[u] || (sorted && k + 1 < n && pn == p);
        vv[u] = need[u] ? col[(uint32_t)wv[u] & 0xFFFFu] : 0.0;
        vp[u] = (lane == 0 && samep[u]) ? col[(uint32_t)we[u] & 0xFFFFu] : 0.0;   // a wave's first lane: its predecessor too
      }
#pragma unroll
      for (int u = 0; u < K0_UB; ++u) {
        if (base0 + u * NT <= ((n >> 6) << 6)) {   // (uniform over the workgroup)
          const int k = base0 + u * NT + tid;
          unsigned long long fk = 0ull;
          if (need[u]) {
            double v = vv[u];
            if (v != v || mask_excluded(ms, v)) v = fill;
            fk = sortable_key(v);
          }
          if (k >= cna && k < n) idx[k] = (uint32_t)wv[u] & 0xFFFFu;
          unsigned long long prev = __shfl_up(fk, 1, 64);   // (read only where samep: the predecessor gathered its key then)
          if (lane == 0 && samep[u]) {
            double v = vp[u];
            if (v != v || mask_excluded(ms, v)) v = fill;
            prev = sortable_key(v);
          }
          // k < cna: inside the fill group; k == cna: the first sorted value, above fill (cna > 0 only when fill < min)
          const bool st = (k <= n) && (k == 0 || k == n || (k >= cna && (!samep[u] || prev != fk)));
          inv |= (samep[u] && prev > fk) ? 1 : 0;
          const unsigned long long b = __ballot(st);
          if (lane == 0 && (k >> 6) <= (n >> 6)) sh_st[k >> 6] = b;
        }
      }
    }
    if (__syncthreads_or(inv) && K0_NETWORK) sort_pass(std::false_type{});
    else starts_done = true;
  }

  // ---- phase 3: tie groups in ascending order -----------------------------------------------------
  // Group starts as a bitset in LDS, computed once with coalesced loads: bit k = "position k starts a tie group";
  // bit n is set (the position after the last one starts a group), so "position k ends a group" is bit k + 1.
  // Every position then finds its group by two bit scans of that set -- first position `lo` = the last start at or
  // before it, last position `hi` = the next start - 1 -- and thread t takes positions t, t + 1024, ...: every
  // global access of the phase is coalesced except the writes by ROW (rec through the LDS tile, hirow).  Round 2a
  // gave each thread a run of consecutive positions: the lanes of a wave then read keys and row indices at a
  // stride of 8 n / 1024 bytes, three key loads per position and pass, and carried the open group from thread to
  // thread with two 1 024-wide LDS scans (K0 without its sort: 0.44 of 1.03 ms on c4).
  if (!starts_done) {
    for (int base = 0; base <= ((n >> 6) << 6); base += NT) {
      const int k = base + tid;
      const bool st = (k <= n) && (k == 0 || k == n || keys[k - 1] != keys[k]);
      const unsigned long long b = __ballot(st);
      if (lane == 0 && (k >> 6) <= (n >> 6)) sh_st[k >> 6] = b;
    }
  }
  unsigned long long* sh_big = reinterpret_cast<unsigned long long*>(sh_ll);  // bit k: a group of >= 2 rows starts at k
  for (int w = tid; w < (WIDE ? pv.Wp : 1024); w += NT) sh_bits[w] = 0ull;
  if (WIDE) {
    for (int k = n + tid; k < pv.n_pad; k += NT) order32[k] = 0u;
  } else {
    for (int k = n + tid; k < pv.n_ord; k += NT) order[k] = 0;  // zero padding: K1 prefetches one step ahead
    if (pv.order_w) { for (int k = n + tid; k < pv.n_ord; k += NT) pv.order_w[(int64_t)c * pv.n_ord + k] = 0u; }
  }
  __syncthreads();
  auto is_start = [&](int k) -> bool { return (sh_st[k >> 6] >> (k & 63)) & 1ull; };   // 0 <= k <= n
  auto prev_start = [&](int k) -> int {   // last start at or before k (bit 0 is set)
    int w = k >> 6;
    unsigned long long m = sh_st[w] & (~0ull >> (63 - (k & 63)));
    while (m == 0ull) m = sh_st[--w];
    return (w << 6) + 63 - (int)__builtin_clzll(m);
  };
  auto next_start = [&](int k) -> int {   // first start after k (bit n is set)
    const int q = k + 1;
    int w = q >> 6;
    unsigned long long m = sh_st[w] & (~0ull << (q & 63));
    while (m == 0ull) m = sh_st[++w];
    return (w << 6) + (int)__builtin_ctzll(m);
  };

  // bit k of sh_big: a tie group of >= 2 rows starts at ascending position k (a start whose successor is not one);
  // sh_bigpre[w]: such groups in the words before w.  A group's rank among them is its place in the column's tie-group
  // list (tgroups, below) and the index every one of its rows carries in girow: the pair kernel counts a streamed
  // group's rows per tie group of the gathered column in a table of counters indexed by it.
  if (!WIDE) {
    const int nw = (n + 63) >> 6;                  // <= 1024 words
    int gbase = 0;                                 // groups in the blocks before this one (the same in every thread)
    for (int wb = 0; wb < nw; wb += NT) {
      const int wi = wb + tid;
      unsigned long long bg = 0ull;
      if (wi < nw) {
        const unsigned long long st = sh_st[wi];
        bg = st & ~((st >> 1) | (sh_st[wi + 1] << 63));
        const int last = n - 1 - wi * 64;          // positions up to n - 1 (bit n of sh_st is the end marker)
        if (last < 63) bg &= (2ull << last) - 1ull;
        sh_big[wi] = bg;
      }
      const int cnt = (int)__popcll(bg);
      const int incl = (int)wave_incl_scan((uint32_t)cnt);
      if (lane == 63) sh_i[tid >> 6] = incl;
      __syncthreads();
      int wbase = gbase, btot = 0;
      for (int w = 0; w < NW; ++w) {
        const int t = sh_i[w];
        if (w < (tid >> 6)) wbase += t;
        btot += t;
      }
      if (wi < nw) sh_bigpre[wi] = (uint16_t)(wbase + incl - cnt);
      gbase += btot;
      __syncthreads();   // (sh_i is rewritten by the next block; the tables are complete for the loop below)
    }
    want_gi = want_gi || gbase > K1_CNT_MIN_GROUPS;
  }

  // per-thread tie statistics over the groups that START at my positions
  int ngroups = 0, maxgroup = 0, tfill = 0, ntg_local = 0, oddtie = 0;
  uint32_t s0 = 0, s1 = 0, s2 = 0;      // int32 arithmetic of Rcpp sugar, as wrapping uint32
  long long e0 = 0, e1 = 0, e2 = 0;     // exact
  for (int base0 = 0; base0 < n; base0 += NT * K0_UB) {
    uint32_t rows[K0_UB];
#pragma unroll
    for (int u = 0; u < K0_UB; ++u) {
      const int k = base0 + u * NT + tid;
      rows[u] = (k < n) ? idx[k] : 0u;
    }
#pragma unroll
    for (int u = 0; u < K0_UB; ++u) {
    if (base0 + u * NT >= n) break;   // (uniform over the workgroup)
    const int k = base0 + u * NT + tid;
    if (k < n) {
      const int lo = prev_start(k), hi = next_start(k) - 1;
      const uint32_t row = rows[u];
      if (WIDE) {
        hi32[row] = (uint32_t)hi; q32[row] = (uint32_t)k; lo32[row] = (uint32_t)lo;
        order32[n - 1 - k] = row;
      } else {
      const uint32_t gi = (want_gi && hi > lo) ? ((uint32_t)sh_bigpre[lo >> 6] + (uint32_t)__popcll(sh_big[lo >> 6] & ((1ull << (lo & 63)) - 1ull)))
                                               : (uint32_t)GIROW_NONE;
      if (stage_hg) hg_s[row] = (uint32_t)hi | (gi << 16);
      else { hirow[2 * row] = (uint16_t)hi; if (want_gi) girow[2 * row] = (uint16_t)gi; }
      // rec is written by row (scattered): through the free sort tile when the column fits, then out in order
      if (stage_rec) rec_s[row] = (uint32_t)k | ((uint32_t)lo << 16);
      else rec[2 * row] = (uint32_t)k | ((uint32_t)lo << 16);
      order[n - 1 - k] = (uint16_t)row;  // processing order of K1: descending value
      if (pv.order_w) pv.order_w[(int64_t)c * pv.n_ord + (n - 1 - k)] = row;
      }
      if (lo == 0 && nna > 0) atomicOr(&sh_bits[row >> 6], 1ull << (row & 63));
      if (lo == k) {
        const int t = hi - lo + 1;
        ++ngroups;
        if (!WIDE) maxgroup = (int)max((uint32_t)maxgroup, ((uint32_t)t << 16) | (uint32_t)lo);  // size << 16 | first position
        if (lo == 0) tfill = t;
        if (t >= 2) {
          ++ntg_local;
          oddtie |= lo & 1;
          const uint32_t ut = (uint32_t)t;
          const uint32_t tt1 = ut * (ut - 1u);
          s0 += tt1;
          s1 += tt1 * (ut - 2u);
          s2 += tt1 * (2u * ut + 5u);
          const long long lt = t;
          e0 += lt * (lt - 1);
          e1 += lt * (lt - 1) * (lt - 2);
          e2 += lt * (lt - 1) * (2 * lt + 5);
        }
      }
    }
    }
  }
  __syncthreads();
  if (stage_rec) {
    for (int r = tid; r < n; r += NT) rec[2 * r] = rec_s[r];
  }
  if (stage_hg) {
    for (int r = tid; r < n; r += NT) {
      const uint32_t hg = hg_s[r];
      hirow[2 * r] = (uint16_t)hg;
      if (want_gi) girow[2 * r] = (uint16_t)(hg >> 16);
    }
  }

  // group-start flags in PROCESSING order k' = n-1-k: a group starts at k' where it ends at k
  for (int base = 0; base < pv.n_pad; base += NT) {
    const int kp = base + tid;
    bool flag = false;
    if (kp < n) {
      const int k = n - 1 - kp;
      flag = is_start(k + 1);
    }
    const unsigned long long b = __ballot(flag);
    if (lane == 0 && (kp >> 6) < W) gflag[kp >> 6] = b;
  }
  if (tid == 0) { gflag[W] = 0ull; }
  for (int w = tid; w <= W; w += NT) fmask[w] = (w < W) ? sh_bits[w] : 0ull;
  int stream_cost = 2 * ((n + 63) >> 6);   // columns without a tie program (long, wide): the steps of their walk
  if (!WIDE && pv.tp_stride > 0) {
    // the tie program of the column: its flag words, still in registers of the lanes that wrote them, go to LDS (the
    // fill-group bitset there has just been copied out) and one wave cuts the steps from that copy
    __syncthreads();
    for (int base = 0; base < pv.n_pad; base += NT) {
      const int kp = base + tid;
      const bool flag = (kp < n) && is_start(n - kp);          // the same bit as above: position n-1-kp ends a group
      const unsigned long long b = __ballot(flag);
      if (lane == 0 && (kp >> 6) < W) sh_bits_lds[kp >> 6] = b;
    }
    if (tid == 0) sh_bits_lds[W] = 0ull;
    __syncthreads();
    // scratch in the sort tile / rec staging area (48 KB, copied out above): E TPROG_WIN u16 | crossT 2 048 u32 | list
    uint16_t* Ewin = reinterpret_cast<uint16_t*>(sh_sort);
    uint32_t* crossT = reinterpret_cast<uint32_t*>(Ewin + TPROG_WIN);
    uint16_t* mlist = reinterpret_cast<uint16_t*>(crossT + 2048);
    k0_tie_program(sh_bits_lds, Ewin, mlist, crossT, &sh_i[0], n, W, pv.tprog + (int64_t)c * pv.tp_stride,
                   pv.tprog + (int64_t)c * pv.tp_stride + (pv.tp_stride - 2 * TPROG_MARKS), order,
                   pv.srow + (int64_t)c * pv.sr_steps * 64, pv.smask + (int64_t)c * pv.sr_steps * 32, pv.sr_steps,
                   (uint32_t)pv.n_pad, tid, NT);
    stream_cost = sh_i[3];   // (every thread reads it; thread 0 stores it with the statistics)
    __syncthreads();   // (sh_i is used by the reductions below)
  }

  // list of the tie groups (size >= 2) in ascending order, lo | hi << 16: K1 counts the joint ties of a
  // tie group of the OTHER column that spans several steps once, when that group closes.  A group's place in the
  // list = the groups of >= 2 rows that start before it: a prefix over the words of sh_big.
  if (!WIDE) {
    const int nw = (n + 63) >> 6;
    for (int wi = tid; wi < nw; wi += NT) {
      int off = (int)sh_bigpre[wi];
      unsigned long long m = sh_big[wi];
      while (m != 0ull) {
        const int k = (wi << 6) + (int)__builtin_ctzll(m);
        m &= m - 1ull;
        tgl[off++] = (uint32_t)k | ((uint32_t)(next_start(k) - 1) << 16);
      }
    }
  }
  // the column's statistics: every value reduced inside its wave, the waves' results combined by thread 0 -- one barrier
  const auto add_i = [](int a, int b) { return a + b; };
  const auto add_u = [](uint32_t a, uint32_t b) { return a + b; };
  const auto add_l = [](long long a, long long b) { return a + b; };
  const int ntg_w = wave_reduce(ntg_local, add_i);
  ngroups = wave_reduce(ngroups, add_i);
  maxgroup = (int)wave_reduce((uint32_t)maxgroup, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
  tfill = wave_reduce(tfill, [](int a, int b) { return a > b ? a : b; });
  oddtie = wave_reduce(oddtie, [](int a, int b) { return a | b; });
  s0 = wave_reduce(s0, add_u); s1 = wave_reduce(s1, add_u); s2 = wave_reduce(s2, add_u);
  e0 = wave_reduce(e0, add_l); e1 = wave_reduce(e1, add_l); e2 = wave_reduce(e2, add_l);
  __syncthreads();   // (sh_i / sh_ll: the list offsets above and the big-group bitset are done with)
  if (lane == 0) {
    int* wi = sh_i + (tid >> 6) * 8;
    wi[0] = ntg_w; wi[1] = ngroups; wi[2] = maxgroup; wi[3] = tfill; wi[4] = oddtie; wi[5] = (int)s0; wi[6] = (int)s1; wi[7] = (int)s2;
    long long* wl = sh_ll + (tid >> 6) * 3;
    wl[0] = e0; wl[1] = e1; wl[2] = e2;
  }
  __syncthreads();
  int ntg = 0;
  if (tid == 0) {
    ngroups = 0; maxgroup = 0; tfill = 0; oddtie = 0; s0 = s1 = s2 = 0u; e0 = e1 = e2 = 0;
    for (int w = 0; w < NW; ++w) {
      const int* wi = sh_i + w * 8;
      ntg += wi[0]; ngroups += wi[1];
      maxgroup = ((uint32_t)wi[2] > (uint32_t)maxgroup) ? wi[2] : maxgroup;
      tfill = max(tfill, wi[3]); oddtie |= wi[4];
      s0 += (uint32_t)wi[5]; s1 += (uint32_t)wi[6]; s2 += (uint32_t)wi[7];
      const long long* wl = sh_ll + w * 3;
      e0 += wl[0]; e1 += wl[1]; e2 += wl[2];
    }
  }

  if (tid == 0) {
    ColStats st;
    st.nna = nna;
    st.ngroups = ngroups;
    st.tfill = (nna > 0) ? tfill : 0;
    st.maxgroup = maxgroup;
    st.s0 = s0; st.s1 = s1; st.s2 = s2; st.ntg = (uint32_t)ntg;
    st.e0 = e0; st.e1 = e1; st.e2 = e2;
    st.fill = fill;
    st.nexcl = nexcl;
    st.flags = (oddtie ? COL_ODD_TIE : 0) | (int32_t)((uint32_t)min(stream_cost, 0xFFFFFF) << 8);
    *pv.col_stats(c) = st;
  }
}

// the kernels of the pre-pass: one body, four shapes (a register budget is a per-kernel attribute)
__global__ void __launch_bounds__(K0_THREADS, ICIKT_K0_MIN_WAVES)
k0_prepare_large(PrepView pv, const double* __restrict__ X, int64_t ld, int col_begin, const MaskSpec ms, uint8_t* __restrict__ keep) {
  k0_prepare_body<false, K0_THREADS, 4>(pv, X, ld, col_begin, ms, keep);
}
// columns of more than 4 096 rows: 8 elements per thread, an 8 192-element tile (96 KB of LDS, 124 KB with the bitsets) --
// half the tiles, one merge level less through the global scratch: 20 000 rows 0.90 -> 0.70 ms per 512 columns, the yeast
// shape 0.090 -> 0.079, 50 000 rows 2.80 -> 2.62 (round 4).  Shorter columns would take the all-LDS path of a partial
// tile there (3 000 rows: 0.19 -> 0.26 ms per 1 024 columns) and keep the 4 096-element tile.
__global__ void __launch_bounds__(K0_THREADS, ICIKT_K0_MIN_WAVES)
k0_prepare_large8(PrepView pv, const double* __restrict__ X, int64_t ld, int col_begin, const MaskSpec ms, uint8_t* __restrict__ keep) {
  k0_prepare_body<false, K0_THREADS, 8>(pv, X, ld, col_begin, ms, keep);
}
__global__ void __launch_bounds__(K0_THREADS, ICIKT_K0_MIN_WAVES)
k0_prepare_wide(PrepView pv, const double* __restrict__ X, int64_t ld, int col_begin, const MaskSpec ms, uint8_t* __restrict__ keep) {
  k0_prepare_body<true, K0_THREADS, K0_TILE / K0_THREADS>(pv, X, ld, col_begin, ms, keep);
}
__global__ void __launch_bounds__(K0_THREADS, ICIKT_K0_WAVES_SMALL)   // (bounds of the LARGE shape: they make the register budget binding; launched with K0_THREADS_SMALL threads)
k0_prepare_small(PrepView pv, const double* __restrict__ X, int64_t ld, int col_begin, const MaskSpec ms, uint8_t* __restrict__ keep) {
  k0_prepare_body<false, K0_THREADS_SMALL, K0_TILE / K0_THREADS_SMALL>(pv, X, ld, col_begin, ms, keep);
}
// two columns in flight on a CU: 512 threads x 8 elements, the 4 096-element tile.  Compiled for four waves per SIMD -- two
// workgroups of eight waves on a CU's four SIMDs -- so it may use 128 VGPRs, and it must not spill: a spilled build of two
// workgroups per CU (64 VGPRs) was what lost 8 % on single-round launches.  Every column length: 9 000 present values
// are two full tiles, a 1 024-element sub-tile and one merge level more through the global scratch than large8 needs.
__global__ void __launch_bounds__(K0_THREADS_PAIR, ICIKT_K0_MIN_WAVES)
k0_prepare_pair(PrepView pv, const double* __restrict__ X, int64_t ld, int col_begin, const MaskSpec ms, uint8_t* __restrict__ keep) {
  k0_prepare_body<false, K0_THREADS_PAIR, K0_TILE / K0_THREADS_PAIR>(pv, X, ld, col_begin, ms, keep);
}

// ------------------------------------------------------------------------------------------------
// K0x: rebuild rec / hirow / tgroups of a column from its order and gflag
// ------------------------------------------------------------------------------------------------
// order (the descending permutation) and gflag (its tie-group starts) determine the other per-row arrays:
// for the row at descending position k, in the group [s, e] of descending positions,
//   q = n-1-k,  lo = n-1-e,  hi = n-1-s   (ascending position, first and last position of its tie group).
// Ranks therefore exchange only order, the three bitsets and stats (24 KB per column of length 10 000 instead
// of 104 KB) and rebuild the rest locally.  One workgroup per column: wave 0 scans the flag words, then the
// waves take the 64-position steps in turn.
constexpr int KX_WAVES = 4;
__global__ void __launch_bounds__(64 * KX_WAVES) k0_expand(PrepView pv, int col_begin, int ncols, int staged) {
  // staged: the scattered per-row writes go to an LDS copy of the column's rec / hirow first and leave as
  // sequential stores (dynamic LDS: n_pad * 8 bytes; the host stages columns of up to 12 288 rows)
  extern __shared__ __attribute__((aligned(16))) unsigned char kx_stage[];
  uint32_t* rec_s = reinterpret_cast<uint32_t*>(kx_stage);
  uint16_t* hi_s = reinterpret_cast<uint16_t*>(kx_stage + (size_t)pv.n_pad * 4);
  uint16_t* gi_s = reinterpret_cast<uint16_t*>(kx_stage + (size_t)pv.n_pad * 6);
  __shared__ __attribute__((aligned(8))) int prevs[1032];   // highest group start in the words before w (-1: none)
  __shared__ int nexts[1032];   // lowest group start in the words after w (n: none)
  __shared__ int msuf[1032];    // groups of size >= 2 that start in the words after w
  __shared__ uint32_t kx_cross[32 * 64];   // k0_tie_program's scratch: cross table, would-be steps, MIXED step list
  __shared__ uint16_t kx_E[TPROG_WIN];
  __shared__ uint16_t kx_list[2 * TPROG_LIST];
  __shared__ int kx_cnt[24];
  const int wave = (int)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const int c = col_begin + (int)blockIdx.x;
  const int n = pv.n, W = pv.W, Wp = pv.Wp;
  const unsigned long long* gf = pv.col_gflag(c);
  const uint16_t* ord = pv.order + (int64_t)c * pv.n_ord;
  uint32_t* rec = pv.rec + ((int64_t)(c >> 1) * pv.rec_rows) * 2 + (c & 1);
  uint16_t* hirow = pv.hirow + ((int64_t)(c >> 1) * pv.rec_rows) * 2 + (c & 1);
  uint16_t* girow = pv.girow + ((int64_t)(c >> 1) * pv.rec_rows) * 2 + (c & 1);
  uint32_t* tgl = pv.tgroups + (int64_t)c * pv.tg_stride;
  if (threadIdx.x == 0) {   // the guard row (PrepView::rec_rows)
    rec[2 * pv.n_pad] = (uint32_t)pv.n_pad; hirow[2 * pv.n_pad] = 0; girow[2 * pv.n_pad] = GIROW_NONE;
  }
  if (pv.order_w) {   // long columns: the received order (with its zero padding) as 32-bit words
    uint32_t* ow = pv.order_w + (int64_t)c * pv.n_ord;
    for (int k = (int)threadIdx.x; k < pv.n_ord; k += (int)blockDim.x) ow[k] = (uint32_t)ord[k];
  }

  // starts of groups of size >= 2: a start whose successor position exists and is not a start
  auto multi = [&](int w) -> unsigned long long {
    const unsigned long long f = gf[w];
    const unsigned long long fn = (f >> 1) | (gf[w + 1] << 63);  // gflag has a zero guard word at W
    unsigned long long m = f & ~fn;
    const int last = n - 2 - w * 64;  // positions k <= n-2 have a successor
    if (last < 63) m &= (last < 0) ? 0ull : ((2ull << last) - 1ull);
    return m;
  };
  if (wave == 0) {
  const int items = (W + 63) >> 6;
  const int w0 = min(W, lane * items), w1 = min(W, w0 + items);
  int hb = -1, lb = n, mc = 0;
  for (int w = w0; w < w1; ++w) {
    const unsigned long long f = gf[w];
    if (f != 0ull) {
      hb = w * 64 + 63 - (int)__builtin_clzll(f);
      if (lb == n) lb = w * 64 + (int)__builtin_ctzll(f);
    }
    mc += (int)__popcll(multi(w));
  }
  // exclusive prefix max of hb, exclusive suffix min of lb, exclusive suffix sum of mc over the lanes
  int pmax = hb, smin = lb, ssum = mc;
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(pmax, o, 64), b = __shfl_down(smin, o, 64), d = __shfl_down(ssum, o, 64);
    if (lane >= o) pmax = max(pmax, a);
    if (lane + o < 64) { smin = min(smin, b); ssum += d; }
  }
  int run_prev = __shfl_up(pmax, 1, 64);
  if (lane == 0) run_prev = -1;
  int run_next = __shfl_down(smin, 1, 64), run_ms = __shfl_down(ssum, 1, 64);
  if (lane == 63) { run_next = n; run_ms = 0; }
  for (int w = w0; w < w1; ++w) {
    prevs[w] = run_prev;
    const unsigned long long f = gf[w];
    if (f != 0ull) run_prev = w * 64 + 63 - (int)__builtin_clzll(f);
  }
  for (int w = w1 - 1; w >= w0; --w) {
    nexts[w] = run_next;
    msuf[w] = run_ms;
    const unsigned long long f = gf[w];
    if (f != 0ull) run_next = w * 64 + (int)__builtin_ctzll(f);
    run_ms += (int)__popcll(multi(w));
  }
  }
  __syncthreads();

  for (int w = wave; w < W; w += KX_WAVES) {
    const int k = w * 64 + lane;
    if (k >= n) break;
    const unsigned long long f = gf[w];
    const unsigned long long le = (lane < 63) ? ((2ull << lane) - 1ull) : ~0ull;  // bits <= lane
    const unsigned long long below = f & le, above = f & ~le;
    const int s = (below != 0ull) ? w * 64 + 63 - (int)__builtin_clzll(below) : prevs[w];
    const int e = ((above != 0ull) ? w * 64 + (int)__builtin_ctzll(above) : nexts[w]) - 1;
    const uint32_t row = ord[k];
    const uint32_t lo = (uint32_t)(n - 1 - e), hi = (uint32_t)(n - 1 - s);
    const uint32_t rv = (uint32_t)(n - 1 - k) | (lo << 16);
    if (staged) { rec_s[row] = rv; hi_s[row] = (uint16_t)hi; }
    else { rec[2 * row] = rv; hirow[2 * row] = (uint16_t)hi; }
    // the group's place in tgroups (ascending in lo: groups that start after it -- descending -- come first), which is
    // the index its rows carry in girow
    uint32_t gi = GIROW_NONE;
    if (e > s) {
      const int sw = s >> 6;
      const unsigned long long les = ((s & 63) < 63) ? ((2ull << (s & 63)) - 1ull) : ~0ull;   // bits <= s
      gi = (uint32_t)(msuf[sw] + (int)__popcll(multi(sw) & ~les));
      if (k == s) tgl[gi] = lo | (hi << 16);
    }
    if (staged) gi_s[row] = (uint16_t)gi;
    else girow[2 * row] = (uint16_t)gi;
  }
  if (staged) {
    __syncthreads();
    for (int r = (int)threadIdx.x; r < n; r += 64 * KX_WAVES) {
      rec[2 * r] = rec_s[r];
      hirow[2 * r] = hi_s[r];
      girow[2 * r] = gi_s[r];
    }
  }
  if (pv.tp_stride > 0) {   // (half-wave kernels only: W <= 287 words)
    __syncthreads();
    unsigned long long* gfl = reinterpret_cast<unsigned long long*>(prevs);   // the scan arrays are free now: 1032 ints = 516 words
    for (int w = (int)threadIdx.x; w <= W; w += 64 * KX_WAVES) gfl[w] = gf[w];
    __syncthreads();
    k0_tie_program(gfl, kx_E, kx_list, kx_cross, kx_cnt, n, W, pv.tprog + (int64_t)c * pv.tp_stride,
                   pv.tprog + (int64_t)c * pv.tp_stride + (pv.tp_stride - 2 * TPROG_MARKS), ord,
                   pv.srow + (int64_t)c * pv.sr_steps * 64, pv.smask + (int64_t)c * pv.sr_steps * 32, pv.sr_steps,
                   (uint32_t)pv.n_pad, (int)threadIdx.x, 64 * KX_WAVES);
  }
}

// ------------------------------------------------------------------------------------------------
// the mask-only pre-pass (pairwise_completeness, R/kendalltau.R:611-629)
// ------------------------------------------------------------------------------------------------
// The mask-only pre-pass: the missing-row bitset of a column and nothing else -- no sort, no statistics.  The
// reference's missing_either (R/kendalltau.R:626-629) never sorts either; the full pre-pass cost 13 ms of sorting per
// c5 matrix here for bitsets that one streaming pass delivers.  One workgroup per (column, slab of 64 words).
constexpr int KM_WORDS = 64;   // words (= waves' 64-row steps) per workgroup: 4 096 rows, 32 KB of the column
__global__ void __launch_bounds__(256)
k0_mask(PrepView pv, const double* __restrict__ X, int64_t ld, int col_begin) {
  const int c = col_begin + (int)blockIdx.x;
  const double* col = X + (int64_t)c * ld;
  unsigned long long* mask = pv.col_mask(c);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int w0 = (int)blockIdx.y * KM_WORDS;
  for (int w = w0 + wave; w < min(w0 + KM_WORDS, pv.W); w += 4) {
    const int i = w * 64 + lane;
    const double v = (i < pv.n) ? col[i] : 0.0;
    const unsigned long long b = __ballot(v != v);
    if (lane == 0) mask[w] = b;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) mask[pv.W] = 0ull;
}

// ------------------------------------------------------------------------------------------------
// launchers (called from icikt_capi.cpp)
// ------------------------------------------------------------------------------------------------
// (every launcher first drops whatever error an earlier, unrelated HIP call of the calling thread left behind: the
//  hipGetLastError() after the launch must report THIS launch)
hipError_t launch_k0(const PrepView& pv, const double* dX, int64_t ld, int col_begin, int ncols, const MaskSpec* msp,
                     uint8_t* keep, int shape, hipStream_t s) {
  (void)hipGetLastError();
  MaskSpec ms{};
  if (msp) ms = *msp;
  if (pv.wide)
    hipLaunchKernelGGL(k0_prepare_wide, dim3(ncols), dim3(K0_THREADS), 0, s, pv, dX, ld, col_begin, ms, keep);
  else if (shape == 1)   // 4 waves per column: fits beside a running pair kernel (the later chunks of the pipelined host path)
    hipLaunchKernelGGL(k0_prepare_small, dim3(ncols), dim3(K0_THREADS_SMALL), 0, s, pv, dX, ld, col_begin, ms, keep);
  else if (shape == 2)   // 8 waves per column, two columns per CU
    hipLaunchKernelGGL(k0_prepare_pair, dim3(ncols), dim3(K0_THREADS_PAIR), 0, s, pv, dX, ld, col_begin, ms, keep);
  else if (pv.npow2 >= 2 * K0_TILE)
    hipLaunchKernelGGL(k0_prepare_large8, dim3(ncols), dim3(K0_THREADS), 0, s, pv, dX, ld, col_begin, ms, keep);
  else
    hipLaunchKernelGGL(k0_prepare_large, dim3(ncols), dim3(K0_THREADS), 0, s, pv, dX, ld, col_begin, ms, keep);
  return hipGetLastError();
}

hipError_t launch_k0_expand(const PrepView& pv, int col_begin, int ncols, hipStream_t s) {
  if (ncols <= 0 || pv.n <= 0) return hipSuccess;
  (void)hipGetLastError();
  const int staged = (pv.n_pad <= 12288) ? 1 : 0;
  const size_t lds = staged ? (size_t)pv.n_pad * 8 : 0;
  if (staged) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k0_expand), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k0_expand, dim3(ncols), dim3(64 * KX_WAVES), lds, s, pv, col_begin, ncols, staged);
  return hipGetLastError();
}

hipError_t launch_k0_mask(const PrepView& pv, const double* dX, int64_t ld, int col_begin, int ncols, hipStream_t s) {
  if (ncols <= 0) return hipSuccess;
  (void)hipGetLastError();
  const unsigned slabs = (unsigned)std::max(1, (pv.W + KM_WORDS - 1) / KM_WORDS);
  hipLaunchKernelGGL(k0_mask, dim3((unsigned)ncols, slabs), dim3(256), 0, s, pv, dX, ld, col_begin);
  return hipGetLastError();
}

}  // namespace icikt
