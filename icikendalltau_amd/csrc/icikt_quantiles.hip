// icikt_quantiles.hip -- exact quantiles and a histogram of raw over all pairs, reduced on the device
// (icikt_quantiles_f64, host side: icikt_capi_quantiles.cpp).
//
// The pair engine runs the combn triangle in blocks of whole rows.  After each block k_quant_fold reads the block's
// records once: it counts every pair into the histogram of its groups (breaks staged in LDS, the bin by binary search,
// LDS-private counters, one flush of the non-zero counters per workgroup), counts valid and NA pairs, and -- when
// quantiles are asked for -- keeps the pair's raw as a sortable 64-bit key (colsort::cor_key, NA_KEY for a pair with a
// reason code) at the pair's place in combn order, as k_median_keep does.  After the last block the host turns n_valid
// into ranks, and a most-significant-digit radix select with 8-bit digits finds the keys of those ranks over the WHOLE
// kept plane: per digit k_quant_count (many workgroups) counts, per live prefix, the next digit of the keys that match
// it, and k_quant_pick (one workgroup) extends every target's prefix by the digit whose bin covers its rank.  Eight
// passes, sixteen launches per batch of targets; all state stays on the device.
//
// Groups: 0 every pair, 1 the pairs with cls[i] == cls[j], 2 the others.  (i, j) is recomputed from the pair's index
// in combn order (q_pair_columns), so nothing but the 8-byte key is kept per pair.  The fold counts groups 0 and 1
// alone: every pair is in exactly one of 1 and 2, so the host takes group 2 as the difference of integers.
//
// Counts are integers added by atomics (LDS, then one global 64-bit atomic per non-zero counter and workgroup): sums of
// integers do not depend on their order, so the result is a pure function of the input, whatever the block cut, the
// batch size or the grid.  No kernel waits on another workgroup; passes are ordered by launch order on one stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"

namespace icikt {

namespace {

using namespace colsort;

// first pair of row i of combn(S, 2) (cut_rows' formula, icikt_blocks.h)
__device__ __forceinline__ long long q_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

// columns (i, j) of pair e of combn(S, 2), 0 <= e < S (S - 1) / 2, S <= 65 535: the row from the root of
// rowoff(i) <= e (the operands stay below 2^35, exact in double), then settled on the integer formula
__device__ __forceinline__ void q_pair_columns(int S, long long e, int* pi, int* pj) {
  const double b = (double)(2 * S - 1);
  int i = (int)((b - sqrt(b * b - 8.0 * (double)e)) * 0.5);
  i = i < 0 ? 0 : (i > S - 2 ? S - 2 : i);
  while (i > 0 && q_rowoff(S, i) > e) --i;
  while (i < S - 2 && q_rowoff(S, i + 1) <= e) ++i;
  *pi = i;
  *pj = i + 1 + (int)(e - q_rowoff(S, i));
}

// ---- fold: histogram, counts and kept keys of one block ----------------------------------------------------------

// slot of a valid raw among nb breaks: 0 below breaks[0], 1 + k in bin k, nb above breaks[nb - 1]; the last bin is
// closed on the right (numpy.histogram)
__device__ __forceinline__ int q_slot(const double* brk, int nb, double v) {
  int lo = 0, hi = nb;   // the number of breaks <= v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (brk[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return (lo == nb && v == brk[nb - 1]) ? nb - 1 : lo;
}

// totals: per counted group c (0: all, 1: within) QUANT_HEAD + nbins words from c * (QUANT_HEAD + nbins) on:
// n_valid, n_na, below, above, then the bins
__global__ void __launch_bounds__(256)
k_quant_fold(const double* __restrict__ out4, const int32_t* __restrict__ reasons, long long n_pairs, long long first,
             int S, const int32_t* __restrict__ cls, const double* __restrict__ breaks, int nb,
             unsigned long long* __restrict__ kept, unsigned long long* __restrict__ totals) {
  __shared__ double s_brk[QUANT_MAX_BINS + 1];
  __shared__ unsigned int s_cnt[2 * (QUANT_MAX_BINS + 2)];   // per counted group: below, the bins, above
  __shared__ unsigned int s_head[4];                         // valid / NA pairs of groups 0 and 1
  const int tid = (int)threadIdx.x;
  const int nslot = nb > 0 ? nb + 1 : 0;
  const int ncg = cls ? 2 : 1;
  for (int q = tid; q < nb; q += 256) s_brk[q] = breaks[q];
  for (int q = tid; q < ncg * nslot; q += 256) s_cnt[q] = 0u;
  if (tid < 4) s_head[tid] = 0u;
  __syncthreads();
  unsigned int nv0 = 0u, nn0 = 0u, nv1 = 0u, nn1 = 0u;
  for (long long base = (long long)blockIdx.x * 256; base < n_pairs; base += (long long)gridDim.x * 256) {
    const long long e = base + tid;
    const bool in = e < n_pairs;
    bool valid = false, within = false;
    double v = 0.0;
    if (in) {
      valid = reasons[e] == 0;
      v = out4[4 * e];
      valid = valid && v == v;   // (a reason-free pair has a raw; cor_key would make NA_KEY of a NaN all the same)
      if (kept) kept[first + e] = valid ? cor_key(v) : NA_KEY;
      if (cls) {
        int i, j;
        q_pair_columns(S, first + e, &i, &j);
        within = cls[i] == cls[j];
      }
    }
    nv0 += (unsigned int)__popcll(__ballot(in && valid));
    nn0 += (unsigned int)__popcll(__ballot(in && !valid));
    if (cls) {
      nv1 += (unsigned int)__popcll(__ballot(in && valid && within));
      nn1 += (unsigned int)__popcll(__ballot(in && !valid && within));
    }
    if (nb > 0) {
      const int slot = (in && valid) ? q_slot(s_brk, nb, v) : -1;
      run_add(s_cnt, slot);
      if (cls) run_add(s_cnt + nslot, within ? slot : -1);
    }
  }
  if ((tid & 63) == 0) {   // the ballots gave every lane the wave's counts
    atomicAdd(&s_head[0], nv0);
    atomicAdd(&s_head[1], nn0);
    atomicAdd(&s_head[2], nv1);
    atomicAdd(&s_head[3], nn1);
  }
  __syncthreads();
  const int stride = QUANT_HEAD + (nb > 0 ? nb - 1 : 0);
  if (tid < 2 * ncg && s_head[tid]) atomicAdd(&totals[(size_t)(tid >> 1) * stride + (tid & 1)], (unsigned long long)s_head[tid]);
  for (int q = tid; q < ncg * nslot; q += 256) {
    const unsigned int n = s_cnt[q];
    if (!n) continue;
    const int c = q / nslot, slot = q - c * nslot;
    // slot 0: below (word 2), slot nb: above (word 3), slot 1 + k: bin k (word QUANT_HEAD + k)
    const int word = slot == 0 ? 2 : (slot == nb ? 3 : QUANT_HEAD + slot - 1);
    atomicAdd(&totals[(size_t)c * stride + word], (unsigned long long)n);
  }
}

// ---- select: the live prefixes of a batch of targets -------------------------------------------------------------

struct QuantSlots {
  unsigned long long pre[QUANT_BATCH_MAX];   // per slot: the prefix (masked), ascending inside a group
  int grp[QUANT_BATCH_MAX];                  // per slot: the group, ascending
  int of[QUANT_BATCH_MAX];                   // per target of the batch: its slot
  int first[QUANT_BATCH_MAX];
  unsigned long long tp[QUANT_BATCH_MAX];
  int tg[QUANT_BATCH_MAX];
  int n;
};

// The distinct (group, prefix & mask) of targets [t0, t0 + nt) in ascending order, nt <= QUANT_BATCH_MAX: the same
// table in the count kernel and in the pick kernel that follows it.  Every thread of the workgroup calls it.
__device__ inline void q_build_slots(QuantSlots& s, const QuantTargets& T, int t0, int nt, unsigned long long mask) {
  const int t = (int)threadIdx.x;
  if (t < nt) {
    s.tp[t] = T.prefix[t0 + t] & mask;
    s.tg[t] = T.group[t0 + t];
  }
  __syncthreads();
  if (t < nt) {
    int f = 1;
    for (int u = 0; u < t; ++u) f &= !(s.tg[u] == s.tg[t] && s.tp[u] == s.tp[t]);
    s.first[t] = f;
  }
  __syncthreads();
  if (t < nt) {
    int r = 0;
    for (int u = 0; u < nt; ++u)
      r += s.first[u] && (s.tg[u] < s.tg[t] || (s.tg[u] == s.tg[t] && s.tp[u] < s.tp[t]));
    s.of[t] = r;
    if (s.first[t]) { s.pre[r] = s.tp[t]; s.grp[r] = s.tg[t]; }
  }
  if (t == 0) {
    int n = 0;
    for (int u = 0; u < nt; ++u) n += s.first[u];
    s.n = n;
  }
  __syncthreads();
}

// the slot of (g, p), or -1
__device__ __forceinline__ int q_find_slot(const QuantSlots& s, int g, unsigned long long p) {
  int lo = 0, hi = s.n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s.grp[mid] < g || (s.grp[mid] == g && s.pre[mid] < p)) lo = mid + 1; else hi = mid;
  }
  return (lo < s.n && s.grp[lo] == g && s.pre[lo] == p) ? lo : -1;
}

// mask of the digits above `shift` (shift 56: none yet)
__device__ __forceinline__ unsigned long long q_mask(int shift) { return shift >= 56 ? 0ull : ~0ull << (shift + 8); }

// hist [slots][256]: += the digit at `shift` of every key whose group and prefix are a live slot's
__global__ void __launch_bounds__(256)
k_quant_count(const unsigned long long* __restrict__ kept, long long n_pairs, int S, const int32_t* __restrict__ cls,
              QuantTargets T, int t0, int nt, int shift, unsigned long long* __restrict__ hist) {
  __shared__ QuantSlots s;
  __shared__ unsigned int s_hist[QUANT_BATCH_MAX * 256];
  const int tid = (int)threadIdx.x;
  const unsigned long long mask = q_mask(shift);
  q_build_slots(s, T, t0, nt, mask);
  const int ns = s.n;
  for (int q = tid; q < ns * 256; q += 256) s_hist[q] = 0u;
  __syncthreads();
  // a workgroup takes a run of whole 256-pair tiles, so a thread's pairs are 256 apart: its (row, place in the row) is
  // found once and then stepped, not recomputed from the index for every key of every pass
  const long long per = ((n_pairs + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
  const long long begin = (long long)blockIdx.x * per;
  const long long end = begin + per < n_pairs ? begin + per : n_pairs;
  int i = 0, off = 0;   // the thread's pair: place `off` of row i, column j = i + 1 + off
  if (cls && begin + tid < end) {
    int j;
    q_pair_columns(S, begin + tid, &i, &j);
    off = j - i - 1;
  }
  // four tiles per step: their four loads are in flight together before the first key is looked up
  constexpr int TILES = 4;
  for (long long base = begin; base < end; base += TILES * 256) {
    unsigned long long keys[TILES];
#pragma unroll
    for (int u = 0; u < TILES; ++u) {
      const long long e = base + u * 256 + tid;
      keys[u] = e < end ? kept[e] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < TILES; ++u) {
      const long long e = base + u * 256 + tid;
      int a = -1, b = -1;
      if (e < end) {
        const unsigned long long key = keys[u];
        const int digit = (int)((key >> shift) & 255ull);
        const int sa = q_find_slot(s, 0, key & mask);
        if (sa >= 0) a = sa * 256 + digit;
        if (cls) {
          const int sb = q_find_slot(s, cls[i] == cls[i + 1 + off] ? 1 : 2, key & mask);
          if (sb >= 0) b = sb * 256 + digit;
        }
      }
      run_add(s_hist, a);
      if (cls) {
        run_add(s_hist, b);
        off += 256;
        while (i < S - 2 && off >= S - 1 - i) {   // (behind the last row nothing is read: e >= end)
          off -= S - 1 - i;
          ++i;
        }
      }
    }
  }
  __syncthreads();
  for (int q = tid; q < ns * 256; q += 256) {
    const unsigned int n = s_hist[q];
    if (n) atomicAdd(&hist[q], (unsigned long long)n);
  }
}

// One workgroup: every target of the batch takes the digit whose bin of its slot's histogram covers its rank; the rank
// becomes the rank inside that bin.  The histograms are zeroed for the next pass.
__global__ void __launch_bounds__(256)
k_quant_pick(QuantTargets T, int t0, int nt, int shift, unsigned long long* __restrict__ hist) {
  __shared__ QuantSlots s;
  __shared__ unsigned long long s_scan[4];
  const int tid = (int)threadIdx.x;
  q_build_slots(s, T, t0, nt, q_mask(shift));
  for (int t = 0; t < nt; ++t) {
    // every thread holds the rank before the scan's barriers: the one thread that writes the reduced rank below does
    // so behind them, and the barrier that ends the iteration keeps it from the next target's reads
    const unsigned long long k = (unsigned long long)T.rank[t0 + t];
    const unsigned long long h = hist[(size_t)s.of[t] * 256 + tid];
    const unsigned long long incl = block_scan(h, s_scan, Add(), 0ull);
    if (incl - h <= k && k < incl) {
      T.prefix[t0 + t] |= (unsigned long long)tid << shift;
      T.rank[t0 + t] = (long long)(k - (incl - h));
    }
    __syncthreads();
  }
  for (int q = tid; q < s.n * 256; q += 256) hist[q] = 0ull;
}

// workgroups of a pass over n_pairs records: the chip eight times over at most
inline unsigned quant_grid(long long n_pairs) {
  const long long want = (n_pairs + 255) / 256;
  return (unsigned)(want < 2048 ? want : 2048);
}

}  // namespace

hipError_t launch_quant_fold(const double* out4, const int32_t* reasons, long long n_pairs, long long first, int S,
                             const int32_t* cls, const double* breaks, int n_breaks, unsigned long long* kept,
                             unsigned long long* totals, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  if (n_breaks < 0 || n_breaks == 1 || n_breaks > QUANT_MAX_BINS + 1 || S < 2 || S > 65535 || first < 0 ||
      first + n_pairs > (long long)S * (S - 1) / 2)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_quant_fold, dim3(quant_grid(n_pairs)), dim3(256), 0, s, out4, reasons, n_pairs, first, S, cls,
                     breaks, n_breaks, kept, totals);
  return hipGetLastError();
}

hipError_t launch_quant_count(const unsigned long long* kept, long long n_pairs, int S, const int32_t* cls,
                              const QuantTargets& T, int t0, int nt, int shift, unsigned long long* hist, hipStream_t s) {
  if (n_pairs <= 0 || nt <= 0) return hipSuccess;
  if (nt > QUANT_BATCH_MAX || shift < 0 || shift > 56 || (shift & 7) || S < 2 || S > 65535 ||
      n_pairs > (long long)S * (S - 1) / 2)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_quant_count, dim3(quant_grid(n_pairs)), dim3(256), 0, s, kept, n_pairs, S, cls, T, t0, nt, shift, hist);
  return hipGetLastError();
}

hipError_t launch_quant_pick(const QuantTargets& T, int t0, int nt, int shift, unsigned long long* hist, hipStream_t s) {
  if (nt <= 0) return hipSuccess;
  if (nt > QUANT_BATCH_MAX || shift < 0 || shift > 56 || (shift & 7)) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_quant_pick, dim3(1), dim3(256), 0, s, T, t0, nt, shift, hist);
  return hipGetLastError();
}

}  // namespace icikt
