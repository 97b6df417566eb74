// icikt_edges.hip -- every pair whose values pass a rule, compacted on the device in combn order (icikt_edges_f64, host
// side: icikt_capi_edges.cpp).
//
// The pair engine runs the combn triangle in blocks of whole rows [row_a, row_b); after each block three launches keep
// the block's matching out4 records, in the block's own order, behind the ones kept so far:
//   k_edge_count   a workgroup per TILE of ED_TILE consecutive pairs: the rule on every record, a ballot word per wave
//                  and round (saved: the write pass reads the MATCHING records only), the tile's count, the degrees;
//   k_edge_scan    ONE workgroup: the exclusive prefix of the tile counts on top of the call's running total (a 64-bit
//                  device word the host zeroes once per call), which it advances;
//   k_edge_write   a workgroup per tile: position = the tile's base + the matches before the thread in the tile; the
//                  record is copied only when that position is below the capacity.
// No kernel waits for another workgroup: the three launches are the synchronisation.  A pair's place in the output is its
// rank among the matching pairs in combn order -- a pure function of the input, whatever the block cut, the tile size or
// the order the workgroups ran in.  k_edge_finish writes the cor plane once max(taumax) is known.
//
// A tile's pairs in its order: round r = 0 .. ED_ROUNDS - 1, thread t = 0 .. 255 -> pair tile * ED_TILE + r * 256 + t.
// A round's 256 pairs are consecutive, so a wave's loads of the 32-byte records are contiguous, and ballot word
// [r][wave] holds 64 consecutive pairs: the order of the words is the order of the pairs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "icikt_device.h"
#include "icikt_wave.h"

namespace icikt {

namespace {

constexpr int ED_THREADS = 256;                       // 4 waves
constexpr int ED_WAVES = ED_THREADS / 64;
constexpr int ED_ROUNDS = 4;                          // records per thread
constexpr int ED_TILE = ED_THREADS * ED_ROUNDS;       // 1 024 pairs
constexpr int ED_WORDS = ED_ROUNDS * ED_WAVES;        // ballot words of a tile
static_assert(ED_WORDS == EDGE_TILE_WORDS, "the host sizes the ballot words by EDGE_TILE_WORDS");

// plain IEEE comparisons: a NaN bound switches its test off, a NaN value fails a test that is on
__device__ __forceinline__ bool edge_match(const EdgeRule& R, double raw, double pval, double comp) {
  bool ok = raw == raw;                               // NA raw (reason codes 1..4): never an edge
  const double v = R.absolute ? fabs(raw) : raw;
  if (R.min_raw == R.min_raw) ok = ok && (v >= R.min_raw);
  if (R.max_pvalue == R.max_pvalue) ok = ok && (pval <= R.max_pvalue);
  if (R.min_completeness == R.min_completeness) ok = ok && (comp >= R.min_completeness);
  return ok;
}

__device__ __forceinline__ long long ed_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

// pair g of combn(S, 2) -> (i, j), 0 <= g < S (S - 1) / 2: the closed form, then a step or two of repair.  Both loops end
// whatever the estimate: ed_rowoff(0) = 0 <= g, ed_rowoff(S - 1) = the number of pairs > g.
__device__ __forceinline__ void ed_pair(long long S, long long g, int& i_out, int& j_out) {
  const double b = 2.0 * (double)S - 1.0;
  long long i = (long long)((b - sqrt(b * b - 8.0 * (double)g)) * 0.5);
  i = max(0ll, min(i, S - 2));
  while (i > 0 && ed_rowoff(S, i) > g) --i;
  while (i < S - 2 && ed_rowoff(S, i + 1) <= g) ++i;
  i_out = (int)i;
  j_out = (int)(i + 1 + (g - ed_rowoff(S, i)));
}

// out4: the block's records; first: the combn index of its first pair; ballots [tiles][ED_WORDS], counts [tiles];
// degree: [S] or nullptr
__global__ void __launch_bounds__(ED_THREADS)
k_edge_count(EdgeRule R, const double* __restrict__ out4, long long n_pairs, long long first, int S,
             unsigned long long* __restrict__ ballots, uint32_t* __restrict__ counts,
             unsigned long long* __restrict__ degree) {
  __shared__ uint32_t s_cnt[ED_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long tile = blockIdx.x;
  uint32_t mine = 0;                                  // lane 0: this wave's matches over the rounds
#pragma unroll
  for (int r = 0; r < ED_ROUNDS; ++r) {
    const long long p = tile * ED_TILE + r * ED_THREADS + tid;
    bool m = false;
    if (p < n_pairs) {
      const double raw = out4[4 * p], pval = out4[4 * p + 1], comp = out4[4 * p + 3];
      m = edge_match(R, raw, pval, comp);
    }
    const unsigned long long b = __ballot(m);         // every lane of the wave is here: no branch above holds one back
    if (lane == 0) ballots[tile * ED_WORDS + r * ED_WAVES + wave] = b;
    mine += (uint32_t)__popcll(b);
    if (degree != nullptr && b != 0ull) {             // (wave-uniform)
      int i = -1, j = -1;
      if (m) ed_pair(S, first + p, i, j);
      // 64 consecutive pairs lie in one row more often than not: then one add carries the row's whole count
      const int i0 = __shfl(i, __ffsll((long long)b) - 1, 64);
      const bool one_row = __all(!m || i == i0);
      if (one_row) {
        if (lane == 0) atomicAdd(&degree[i0], (unsigned long long)__popcll(b));
      } else if (m) {
        atomicAdd(&degree[i], 1ull);
      }
      if (m) atomicAdd(&degree[j], 1ull);
    }
  }
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  if (tid == 0) counts[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// bases[t] = *total + counts[0] + .. + counts[t - 1]; *total += the sum of the counts.  One workgroup.
__global__ void __launch_bounds__(ED_THREADS)
k_edge_scan(const uint32_t* __restrict__ counts, long long n_tiles, unsigned long long* __restrict__ bases,
            unsigned long long* __restrict__ total) {
  __shared__ uint32_t s_w[ED_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long running = *total;                // read by every thread before thread 0 writes it (behind the last barrier)
  for (long long c0 = 0; c0 < n_tiles; c0 += ED_THREADS) {   // (the trip count is the same for every thread)
    const long long t = c0 + tid;
    const uint32_t v = t < n_tiles ? counts[t] : 0u;
    const uint32_t incl = wave_incl_scan(v);          // <= 64 x 1 024
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    const uint32_t w0 = s_w[0], w1 = s_w[1], w2 = s_w[2], w3 = s_w[3];
    __syncthreads();                                  // s_w is free for the next trip
    const uint32_t before = (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
    if (t < n_tiles) bases[t] = running + before + (incl - v);
    running += (unsigned long long)w0 + w1 + w2 + w3;
  }
  if (tid == 0) *total = running;
}

__global__ void __launch_bounds__(ED_THREADS)
k_edge_write(const double* __restrict__ out4, long long n_pairs, long long first, int S,
             const unsigned long long* __restrict__ ballots, const uint32_t* __restrict__ counts,
             const unsigned long long* __restrict__ bases, EdgeOut E) {
  __shared__ unsigned long long s_b[ED_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long tile = blockIdx.x;
  const unsigned long long base = bases[tile];
  // (both the same for every thread of the workgroup) nothing matched, or the tile starts past the capacity
  if (counts[tile] == 0u || base >= (unsigned long long)E.cap) return;
  if (tid < ED_WORDS) s_b[tid] = ballots[tile * ED_WORDS + tid];
  __syncthreads();
  uint32_t before = 0;                                // matches in the words ahead of this thread's word of round 0
  for (int w = 0; w < wave; ++w) before += (uint32_t)__popcll(s_b[w]);
#pragma unroll
  for (int r = 0; r < ED_ROUNDS; ++r) {
    const unsigned long long b = s_b[r * ED_WAVES + wave];
    if ((b >> lane) & 1ull) {
      const unsigned long long at = base + before + (uint32_t)__popcll(b & low_mask64((uint32_t)lane));
      if (at < (unsigned long long)E.cap) {
        const long long p = tile * ED_TILE + r * ED_THREADS + tid;   // < n_pairs: the count pass set the bit
        int i, j;
        ed_pair(S, first + p, i, j);
        const double raw = out4[4 * p], pval = out4[4 * p + 1], tmax = out4[4 * p + 2], comp = out4[4 * p + 3];
        E.ei[at] = i;
        E.ej[at] = j;
        E.raw[at] = raw;
        E.pvalue[at] = pval;
        E.taumax[at] = tmax;
        E.completeness[at] = comp;
      }
    }
    // on to the same wave's word of the next round: the rest of this round's words and the next round's first ones
    if (r + 1 < ED_ROUNDS)
      for (int w = 0; w < ED_WAVES; ++w) before += (uint32_t)__popcll(s_b[r * ED_WAVES + wave + w]);
  }
}

// cor of the first n kept edges: k_assemble's expression on k_assemble's operands
__global__ void __launch_bounds__(256)
k_edge_finish(EdgeOut E, long long n, const unsigned long long* __restrict__ red, int scale_max) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const unsigned long long k = red[0];
  // max(numeric(0), na.rm = TRUE) is -Inf in R
  const double max_cor = k ? __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k))
                           : -__longlong_as_double(0x7FF0000000000000ll);
  const double raw = E.raw[t];
  E.cor[t] = scale_max ? raw / max_cor : raw;
}

}  // namespace

long long edge_tiles(long long n_pairs) { return (n_pairs + ED_TILE - 1) / ED_TILE; }

hipError_t launch_edge_block(const EdgeRule& R, const double* out4, long long n_pairs, long long first, int S,
                             unsigned long long* ballots, uint32_t* counts, unsigned long long* bases,
                             unsigned long long* total, unsigned long long* degree, const EdgeOut& E, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  const long long all = (long long)S * (S - 1) / 2;
  if (S < 2 || S > 65535 || first < 0 || first + n_pairs > all || E.cap < 0) return hipErrorInvalidValue;
  const long long tiles = edge_tiles(n_pairs);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_edge_count, dim3((unsigned)tiles), dim3(ED_THREADS), 0, s, R, out4, n_pairs, first, S, ballots,
                     counts, degree);
  hipLaunchKernelGGL(k_edge_scan, dim3(1), dim3(ED_THREADS), 0, s, counts, tiles, bases, total);
  if (E.cap > 0)
    hipLaunchKernelGGL(k_edge_write, dim3((unsigned)tiles), dim3(ED_THREADS), 0, s, out4, n_pairs, first, S, ballots,
                       counts, bases, E);
  return hipGetLastError();
}

hipError_t launch_edge_finish(const EdgeOut& E, long long n, const unsigned long long* red, int scale_max, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > E.cap) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_edge_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, E, n, red, scale_max);
  return hipGetLastError();
}

}  // namespace icikt
