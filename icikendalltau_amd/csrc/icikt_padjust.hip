// icikt_padjust.hip -- multiple-testing adjustment of the p-values of all pairs, on the device (icikt_padjust_f64, host
// side: icikt_capi_padjust.cpp).
//
// The pair engine runs the combn triangle in blocks of whole rows.  After each block k_padj_fold keeps every pair's
// p-value as a sortable 64-bit key (colsort::cor_key; NA_KEY for a pair with a reason code or a NaN p) at the pair's
// place in combn order, counts the valid keys, and counts every key's eight digits into one [8][256] table.  After the
// last block the whole plane is sorted ascending, NA keys last, by a least-significant-digit radix sort with 8-bit
// digits between the kept plane and a spare one: per digit k_padj_hist (the digit histogram of every tile),
// a scan of the (digit, tile) counts, and k_padj_scatter (stable).  The host skips a digit that the fold's table
// shows to be the same in all keys.  A tile is a run of consecutive keys that ONE WAVE takes 64 at a time, in order: a
// key's place among the keys of its digit is a count over the wave's ballots and the wave's running offsets, so
// nothing in the scatter waits for another wave.
//
// Over the first m sorted positions (m: the valid keys) the adjusted values are a scan of exact operations: the key
// decoded and multiplied by the method's factor of its position (one division and one multiplication, each rounded on
// its own; no addition of doubles, so nothing contracts), then a running maximum (Holm), a running minimum from the
// right (Hochberg, BH) or nothing (Bonferroni), clamped at 1, written over the sort's spare plane.  k_padj_cut finds per
// alpha the number of adjusted values <= alpha by binary search (the plane is non-decreasing), and the table of distinct
// p-values with their adjusted values is an ordered compaction of the heads of runs of equal keys.
//
// Every chip-wide scan here (the sort's offsets, the running minimum / maximum, the table's places) is the same three
// launches: k_scan_agg (each chunk of PADJ_SCAN_CHUNK items reduced), k_scan_top (ONE workgroup turns the chunks'
// aggregates into their exclusive prefixes, 256 at a time with a carry), k_scan_apply (each chunk scanned again behind
// its prefix).  No kernel waits on another workgroup; phases are ordered by kernel boundaries on one stream.  Integer
// sums, minima and maxima do not depend on their order, so the result is a pure function of the input, whatever the
// block cut, the tile or the grid.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_select.h"

namespace icikt {

namespace {

using namespace colsort;

constexpr int SCAN_ITEMS = PADJ_SCAN_CHUNK / CT;   // consecutive items of a thread
static_assert(SCAN_ITEMS * CT == PADJ_SCAN_CHUNK, "a chunk is a whole number of items per thread");

// ---- fold: the kept keys, the valid count and the digit table of one block ---------------------------------------

__global__ void __launch_bounds__(256)
k_padj_fold(const double* __restrict__ out4, const int32_t* __restrict__ reasons, long long n_pairs, long long first,
            unsigned long long* __restrict__ kept, unsigned long long* __restrict__ total,
            unsigned long long* __restrict__ dhist) {
  __shared__ unsigned int s_hist[8 * 256];
  __shared__ unsigned int s_valid;
  const int tid = (int)threadIdx.x;
  for (int q = tid; q < 8 * 256; q += 256) s_hist[q] = 0u;
  if (tid == 0) s_valid = 0u;
  __syncthreads();
  unsigned int nv = 0u;
  for (long long base = (long long)blockIdx.x * 256; base < n_pairs; base += (long long)gridDim.x * 256) {
    const long long e = base + tid;
    const bool in = e < n_pairs;
    bool valid = false;
    unsigned long long key = NA_KEY;
    if (in) {
      const double p = out4[4 * e + 1];
      valid = reasons[e] == 0 && p == p;   // (2-row input: a reason-free pair whose p is NaN, dropped as p.adjust drops it)
      if (valid) key = cor_key(p);
      kept[first + e] = key;
    }
    nv += (unsigned int)__popcll(__ballot(in && valid));
#pragma unroll
    for (int d = 0; d < 8; ++d) run_add(s_hist + d * 256, in ? (int)((key >> (8 * d)) & 255ull) : -1);
  }
  if ((tid & 63) == 0) atomicAdd(&s_valid, nv);   // the ballots gave every lane the wave's count
  __syncthreads();
  if (tid == 0 && s_valid) atomicAdd(total, (unsigned long long)s_valid);
  for (int q = tid; q < 8 * 256; q += 256) {
    const unsigned int n = s_hist[q];
    if (n) atomicAdd(&dhist[q], (unsigned long long)n);
  }
}

// ---- sort: one digit of the radix sort ---------------------------------------------------------------------------

// counts [256][n_tiles]: the keys of tile t (keys [t * tile, min((t + 1) * tile, n)), one wave's) with digit d
__global__ void __launch_bounds__(256)
k_padj_hist(const unsigned long long* __restrict__ src, long long n, long long tile, long long n_tiles, int shift,
            unsigned long long* __restrict__ counts) {
  __shared__ unsigned int s_h[4][256];
  const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
  for (long long t0 = (long long)blockIdx.x * 4; t0 < n_tiles; t0 += (long long)gridDim.x * 4) {
    const long long t = t0 + w;   // (the wave's tile; the trip count is the workgroup's)
    for (int q = lane; q < 256; q += 64) s_h[w][q] = 0u;
    __syncthreads();
    if (t < n_tiles) {
      const long long begin = t * tile, end = begin + tile < n ? begin + tile : n;
      for (long long b = begin; b < end; b += 64) {
        const long long e = b + lane;
        run_add(s_h[w], e < end ? (int)((src[e] >> shift) & 255ull) : -1);
      }
    }
    __syncthreads();
    if (t < n_tiles)
      for (int q = lane; q < 256; q += 64) counts[(long long)q * n_tiles + t] = (unsigned long long)s_h[w][q];
    __syncthreads();
  }
}

// offsets [256][n_tiles]: where the first key of tile t with digit d goes (the exclusive scan of k_padj_hist's counts).
// Stable: a wave takes its tile 64 keys at a time in order, and inside a step a key's place among the keys of its
// digit is its rank among the lanes that hold that digit.
__global__ void __launch_bounds__(256)
k_padj_scatter(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, long long n,
               long long tile, long long n_tiles, int shift, const unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long s_off[4][256];
  const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
  // (read and written by different lanes of ONE wave from step to step: LDS operations of a wave complete in order)
  volatile unsigned long long* const off = s_off[w];
  for (long long t0 = (long long)blockIdx.x * 4; t0 < n_tiles; t0 += (long long)gridDim.x * 4) {
    const long long t = t0 + w;
    if (t < n_tiles)
      for (int q = lane; q < 256; q += 64) off[q] = offsets[(long long)q * n_tiles + t];
    __syncthreads();
    if (t < n_tiles) {
      const long long begin = t * tile, end = begin + tile < n ? begin + tile : n;
      for (long long b = begin; b < end; b += 64) {
        const long long e = b + lane;
        const bool in = e < end;
        const unsigned long long key = in ? src[e] : 0ull;
        const int d = (int)((key >> shift) & 255ull);
        unsigned long long peers = __ballot(in);   // the lanes that hold a key with this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
          const bool one = (d >> bit) & 1;
          const unsigned long long vote = __ballot(in && one);
          peers &= one ? vote : ~vote;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        unsigned long long base = 0ull;
        if (in && rank == 0) {   // the digit's first lane moves the wave's offset past the step's keys
          base = off[d];
          off[d] = base + (unsigned long long)__popcll(peers);
        }
        const int leader = in ? __ffsll((long long)peers) - 1 : lane;
        base = __shfl(base, leader, 64);
        if (in && base + (unsigned long long)rank < (unsigned long long)n) dst[base + (unsigned long long)rank] = key;
      }
    }
    __syncthreads();
  }
}

// ---- the chip-wide scan: chunk aggregates, one workgroup over them, apply -----------------------------------------

__device__ __forceinline__ long long scan_extent(long long n_host, const unsigned long long* n_dev) {
  if (!n_dev) return n_host;
  const long long d = (long long)*n_dev;
  return d < n_host ? d : n_host;
}

// agg[c] = the op of the items of chunk c (PADJ_SCAN_CHUNK items, the last chunk fewer); n_dev (may be null): a
// device word that bounds the extent from below n_host
template <typename T, typename Op, typename Src>
__global__ void __launch_bounds__(256)
k_scan_agg(Src src, long long n_host, const unsigned long long* __restrict__ n_dev, T ident, T* __restrict__ agg) {
  __shared__ T sh[4];
  const long long n = scan_extent(n_host, n_dev);
  const long long n_chunks = (n + PADJ_SCAN_CHUNK - 1) / PADJ_SCAN_CHUNK;
  Op op;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const long long i0 = c * PADJ_SCAN_CHUNK + (long long)threadIdx.x * SCAN_ITEMS;
    T v = ident;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
      if (i0 + k < n) v = op(v, src(i0 + k));
    v = block_reduce(v, sh, op);
    if (threadIdx.x == 0) agg[c] = v;
  }
}

// One workgroup: agg[c] becomes the op of the chunks before c (ident for c = 0), *total (may be null) the op of all
template <typename T, typename Op>
__global__ void __launch_bounds__(256)
k_scan_top(T* __restrict__ agg, long long n_host, const unsigned long long* __restrict__ n_dev, T ident,
           T* __restrict__ total) {
  __shared__ T sh[4];
  __shared__ T s_incl[CT];
  const long long n = scan_extent(n_host, n_dev);
  const long long n_chunks = (n + PADJ_SCAN_CHUNK - 1) / PADJ_SCAN_CHUNK;
  const int tid = (int)threadIdx.x;
  Op op;
  T carry = ident;
  for (long long b = 0; b < n_chunks; b += CT) {
    const long long i = b + tid;
    const T v = i < n_chunks ? agg[i] : ident;
    const T incl = block_scan(v, sh, op, ident);
    s_incl[tid] = incl;
    __syncthreads();
    const T excl = tid ? s_incl[tid - 1] : ident;
    const T all = s_incl[CT - 1];
    if (i < n_chunks) agg[i] = op(carry, excl);
    carry = op(carry, all);
    __syncthreads();
  }
  if (tid == 0 && total) *total = carry;
}

// dst(i, v, incl) for every item i < n: v the item, incl the op of the items 0 .. i
template <typename T, typename Op, typename Src, typename Dst>
__global__ void __launch_bounds__(256)
k_scan_apply(Src src, Dst dst, long long n_host, const unsigned long long* __restrict__ n_dev, T ident,
             const T* __restrict__ agg) {
  __shared__ T sh[4];
  __shared__ T s_incl[CT];
  const long long n = scan_extent(n_host, n_dev);
  const long long n_chunks = (n + PADJ_SCAN_CHUNK - 1) / PADJ_SCAN_CHUNK;
  const int tid = (int)threadIdx.x;
  Op op;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const long long i0 = c * PADJ_SCAN_CHUNK + (long long)tid * SCAN_ITEMS;
    T v[SCAN_ITEMS];
    T mine = ident;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      v[k] = i0 + k < n ? src(i0 + k) : ident;
      mine = op(mine, v[k]);
    }
    const T incl = block_scan(mine, sh, op, ident);
    s_incl[tid] = incl;
    __syncthreads();
    T run = op(agg[c], tid ? s_incl[tid - 1] : ident);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      run = op(run, v[k]);
      if (i0 + k < n) dst(i0 + k, v[k], run);
    }
  }
}

// the sort's offsets: an exclusive sum in place
struct CountSrc {
  const unsigned long long* counts;
  __device__ unsigned long long operator()(long long i) const { return counts[i]; }
};
struct OffsetDst {
  unsigned long long* offsets;
  __device__ void operator()(long long i, unsigned long long v, unsigned long long incl) const { offsets[i] = incl - v; }
};

// ---- adjust -------------------------------------------------------------------------------------------------------

// the method's factor of the 0-based sorted position pos among m tests, times p: R's p.adjust, one IEEE operation at
// a time (m, pos + 1 and m - pos are below 2^31: exact as doubles)
__device__ __forceinline__ double pa_scaled(int method, long long m, long long pos, double p) {
#pragma clang fp contract(off)
  if (method == PADJ_BH) {
    const double q = (double)m / (double)(pos + 1);
    return q * p;
  }
  const double f = method == PADJ_BONFERRONI ? (double)m : (double)(m - pos);
  return f * p;
}

// item i of the scan is sorted position i (Holm: a running maximum from the left) or m - 1 - i (Hochberg, BH: a
// running minimum from the right)
struct AdjustSrc {
  const unsigned long long* keys;
  long long m;
  int method;
  __device__ long long pos(long long i) const { return method == PADJ_HOLM ? i : m - 1 - i; }
  __device__ double operator()(long long i) const {
    const long long q = pos(i);
    return pa_scaled(method, m, q, sel::key_value(keys[q]));
  }
};
struct AdjustDst {
  double* adj;
  long long m;
  int method;
  __device__ void operator()(long long i, double, double incl) const {
    adj[method == PADJ_HOLM ? i : m - 1 - i] = incl < 1.0 ? incl : 1.0;
  }
};

__global__ void __launch_bounds__(256)
k_padj_bonferroni(const unsigned long long* __restrict__ keys, long long m, double* __restrict__ adj) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
    const double v = pa_scaled(PADJ_BONFERRONI, m, i, sel::key_value(keys[i]));
    adj[i] = v < 1.0 ? v : 1.0;
  }
}

// ---- cut-offs and table --------------------------------------------------------------------------------------------

// cut [2 * PADJ_MAX_ALPHA + 1]: per alpha the adjusted values <= alpha (adj is non-decreasing: the first position
// above alpha), then per alpha the bits of the largest rejected p (NA_real_ when none), then the largest count
__global__ void __launch_bounds__(64)
k_padj_cut(const double* __restrict__ adj, const unsigned long long* __restrict__ keys, long long m,
           const double* __restrict__ alpha, int n_alpha, unsigned long long* __restrict__ cut) {
  __shared__ unsigned long long s_n[PADJ_MAX_ALPHA];
  const int tid = (int)threadIdx.x;
  if (tid < n_alpha) {
    const double a = alpha[tid];
    long long lo = 0, hi = m;
    while (lo < hi) {
      const long long mid = lo + ((hi - lo) >> 1);
      if (adj[mid] <= a) lo = mid + 1; else hi = mid;
    }
    s_n[tid] = (unsigned long long)lo;
    cut[tid] = (unsigned long long)lo;
    cut[PADJ_MAX_ALPHA + tid] =
        lo > 0 ? (unsigned long long)__double_as_longlong(sel::key_value(keys[lo - 1])) : sel::R_NA_BITS;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long most = 0ull;
    for (int a = 0; a < n_alpha; ++a) most = s_n[a] > most ? s_n[a] : most;
    cut[2 * PADJ_MAX_ALPHA] = most;
  }
}

// the heads of runs of equal keys among the sorted keys, each stored at its rank among the heads while there is room
struct HeadSrc {
  const unsigned long long* keys;
  __device__ unsigned long long operator()(long long i) const { return (i == 0 || keys[i] != keys[i - 1]) ? 1ull : 0ull; }
};
struct TableDst {
  const unsigned long long* keys;
  const double* adj;
  double* table;   // [2][cap]
  long long cap;
  __device__ void operator()(long long i, unsigned long long head, unsigned long long incl) const {
    if (!head) return;
    const long long at = (long long)incl - 1;
    if (at < cap) {
      table[at] = sel::key_value(keys[i]);
      table[cap + at] = adj[i];
    }
  }
};

inline unsigned scan_grid(long long n) {
  const long long want = (n + PADJ_SCAN_CHUNK - 1) / PADJ_SCAN_CHUNK;
  return (unsigned)(want < 1 ? 1 : (want < 4096 ? want : 4096));
}

// the three launches of a scan over n_host items (n_dev: see k_scan_agg)
template <typename T, typename Op, typename Src, typename Dst>
hipError_t run_scan(Src src, Dst dst, long long n_host, const unsigned long long* n_dev, T ident, T* agg, T* total,
                    hipStream_t s) {
  (void)hipGetLastError();
  const unsigned grid = scan_grid(n_host);
  hipLaunchKernelGGL((k_scan_agg<T, Op, Src>), dim3(grid), dim3(256), 0, s, src, n_host, n_dev, ident, agg);
  hipLaunchKernelGGL((k_scan_top<T, Op>), dim3(1), dim3(256), 0, s, agg, n_host, n_dev, ident, total);
  hipLaunchKernelGGL((k_scan_apply<T, Op, Src, Dst>), dim3(grid), dim3(256), 0, s, src, dst, n_host, n_dev, ident, agg);
  return hipGetLastError();
}

}  // namespace

long long padj_tile(long long n, long long want) {
  long long tile = want > 0 ? want : 1024;
  const long long least = (n + PADJ_MAX_TILES - 1) / PADJ_MAX_TILES;
  if (tile < least) tile = want > 0 ? least : (least + 63) / 64 * 64;
  return tile < 1 ? 1 : tile;
}

long long padj_scan_chunks(long long n, long long tile) {
  const long long n_tiles = tile > 0 ? (n + tile - 1) / tile : 0;
  const long long items = 256 * n_tiles > n ? 256 * n_tiles : n;
  return (items + PADJ_SCAN_CHUNK - 1) / PADJ_SCAN_CHUNK + 1;
}

hipError_t launch_padj_fold(const double* out4, const int32_t* reasons, long long n_pairs, long long first, int S,
                            unsigned long long* kept, unsigned long long* total, unsigned long long* dhist,
                            hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  if (S < 2 || S > 65535 || first < 0 || first + n_pairs > (long long)S * (S - 1) / 2) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const long long want = (n_pairs + 255) / 256;
  hipLaunchKernelGGL(k_padj_fold, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, s, out4, reasons, n_pairs,
                     first, kept, total, dhist);
  return hipGetLastError();
}

hipError_t launch_padj_sort_pass(const unsigned long long* src, unsigned long long* dst, long long n, long long tile,
                                 int shift, unsigned long long* counts, unsigned long long* agg, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (tile < 1 || shift < 0 || shift > 56 || (shift & 7) || src == dst) return hipErrorInvalidValue;
  const long long n_tiles = (n + tile - 1) / tile;
  if (n_tiles > PADJ_MAX_TILES) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const long long want = (n_tiles + 3) / 4;
  const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(k_padj_hist, dim3(grid), dim3(256), 0, s, src, n, tile, n_tiles, shift, counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = run_scan<unsigned long long, Add>(CountSrc{counts}, OffsetDst{counts}, 256 * n_tiles, nullptr, 0ull, agg,
                                        (unsigned long long*)nullptr, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_padj_scatter, dim3(grid), dim3(256), 0, s, src, dst, n, tile, n_tiles, shift, counts);
  return hipGetLastError();
}

hipError_t launch_padj_adjust(const unsigned long long* keys, long long m, int method, double* adj, double* agg,
                              hipStream_t s) {
  if (m <= 0) return hipSuccess;
  if (m > 0x7FFFFFFFll) return hipErrorInvalidValue;
  (void)hipGetLastError();
  if (method == PADJ_BONFERRONI) {
    const long long want = (m + 255) / 256;
    hipLaunchKernelGGL(k_padj_bonferroni, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, keys, m, adj);
    return hipGetLastError();
  }
  const AdjustSrc src{keys, m, method};
  const AdjustDst dst{adj, m, method};
  const double inf = __builtin_huge_val();
  if (method == PADJ_HOLM) return run_scan<double, Max>(src, dst, m, nullptr, -inf, agg, (double*)nullptr, s);
  if (method == PADJ_HOCHBERG || method == PADJ_BH)
    return run_scan<double, Min>(src, dst, m, nullptr, inf, agg, (double*)nullptr, s);
  return hipErrorInvalidValue;
}

hipError_t launch_padj_cut(const double* adj, const unsigned long long* keys, long long m, const double* alpha,
                           int n_alpha, unsigned long long* cut, hipStream_t s) {
  if (m <= 0 || n_alpha < 1 || n_alpha > PADJ_MAX_ALPHA) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_padj_cut, dim3(1), dim3(64), 0, s, adj, keys, m, alpha, n_alpha, cut);
  return hipGetLastError();
}

hipError_t launch_padj_table(const unsigned long long* keys, const double* adj, long long m,
                             const unsigned long long* extent, long long cap, double* table, unsigned long long* agg,
                             unsigned long long* n_table, hipStream_t s) {
  if (m <= 0 || cap < 0 || !extent || !n_table) return hipErrorInvalidValue;
  return run_scan<unsigned long long, Add>(HeadSrc{keys}, TableDst{keys, adj, table, cap}, m, extent, 0ull, agg,
                                           n_table, s);
}

}  // namespace icikt
