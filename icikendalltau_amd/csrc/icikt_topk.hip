// icikt_topk.hip -- top-k partners per sample, selected on the device (icikt_topk_f64, host side: icikt_capi_topk.cpp).
//
// The pair engine runs the combn triangle in blocks of whole rows [row_a, row_b); after each block k_topk_merge folds
// the block's out4 records into every column's running list of its k best partners, and k_topk_finish writes the
// lists out once the last block is through.  Nothing here is of size S^2.
//
// The order of a column's list is STRICT: raw descending in the total order of the sortable key (-0.0 below +0.0),
// ties by the smaller partner index; partner indices are unique within a column.  The threshold test, the compaction
// and the sort all go through tk_before(), so the result is a pure function of the set of (raw, partner) and does not
// depend on how the triangle was cut into blocks.
//
// A column's list lives in global memory twice (TopkLists: two buffers, `cur` says which one is current): a block's
// out4 is gone after the block, so the four doubles of a kept pair are copied beside its entry when the merged list is
// written -- into the buffer that is NOT current, because the merged list reads its payloads from the current one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "icikt_device.h"

namespace icikt {

namespace {

constexpr int TK_THREADS = 256;        // one workgroup (4 waves) per column
constexpr int TK_CAP = 256;            // == ICIKT_TOPK_MAX: entries of a list, and of the survivor buffer behind it
constexpr int TK_SENTINEL_PARTNER = 0x7FFFFFFF;

// monotone in v; 0 is below every double (dbl_sortable of icikt_epilogue.hip)
__device__ __forceinline__ unsigned long long tk_sortable(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double tk_unsortable(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
// the list's strict order: does (ka, pa) come before (kb, pb)?
__device__ __forceinline__ bool tk_before(unsigned long long ka, int32_t pa, unsigned long long kb, int32_t pb) {
  return ka > kb || (ka == kb && pa < pb);
}
// first pair of row i of combn(S, 2)
__device__ __forceinline__ long long tk_rowoff(long long S, long long i) { return i * (2 * S - i - 1) / 2; }

// One workgroup per column c = row_a + blockIdx.x (the columns below row_a have no pair in this block).  Column c's
// candidates in the block are the strided records (i, c), i in [row_a, min(row_b, c)), and, when row_a <= c < row_b, the
// contiguous row (c, c + 1 .. S - 1).  LDS: entries [0, 256) the list (sorted, nlist of them), [256, 512) the survivors
// of this block that beat the list's k-th entry; as three arrays (8-byte keys, 4-byte partners, 4-byte payload sources)
// so that every access is a plain b64 / b32 one.  src >= 0: the block-relative pair whose out4 record holds the
// payload; src < 0: slot ~src of the current global list.
__global__ void __launch_bounds__(TK_THREADS)
k_topk_merge(TopkLists L, const double* __restrict__ out4, int S, int row_a, int row_b, long long base) {
  __shared__ unsigned long long s_key[2 * TK_CAP];
  __shared__ int32_t s_part[2 * TK_CAP];
  __shared__ int32_t s_src[2 * TK_CAP];
  __shared__ int s_wcnt[2][TK_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = row_a + (int)blockIdx.x;
  const int k = L.k;
  const int n_col = min(row_b, c) - row_a;
  const int n_row = (c < row_b) ? S - 1 - c : 0;
  const int T = n_col + n_row;
  if (c >= S || T <= 0) return;   // (the same for every thread of the workgroup)
  const int cur = L.cur[c];
  int nlist = L.count[c];
  const size_t old_at = ((size_t)cur * (size_t)S + (size_t)c) * (size_t)k;
  if (tid < nlist) {
    s_key[tid] = L.key[old_at + tid];
    s_part[tid] = L.partner[old_at + tid];
    s_src[tid] = ~tid;
  }
  __syncthreads();
  unsigned long long thr_key = 0ull;
  int32_t thr_part = TK_SENTINEL_PARTNER;
  if (nlist == k) { thr_key = s_key[k - 1]; thr_part = s_part[k - 1]; }
  int nbuf = 0, par = 0;
  bool changed = false;
  const long long row_c = tk_rowoff(S, c) - base;

  // list U buffer -> the first min(k, nlist + nbuf) of their union in the list's order.  Every thread runs it with the
  // same nlist / nbuf (they are kept in registers, derived from workgroup-uniform values only).
  auto flush = [&]() {
    __syncthreads();   // the buffer's entries are written
    for (int i = tid; i < 2 * TK_CAP; i += TK_THREADS)
      if ((i >= nlist && i < TK_CAP) || i >= TK_CAP + nbuf) {
        s_key[i] = 0ull;   // below every candidate: NaN is dropped before it gets a key
        s_part[i] = TK_SENTINEL_PARTNER;
        s_src[i] = 0;
      }
    __syncthreads();
    for (int size = 2; size <= 2 * TK_CAP; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        const int i = ((tid & ~(stride - 1)) << 1) | (tid & (stride - 1)), j = i + stride;
        const unsigned long long ka = s_key[i], kb = s_key[j];
        const int32_t pa = s_part[i], pb = s_part[j];
        const bool fwd = (i & size) == 0;   // this run ends in the list's order (else in its reverse)
        if (fwd ? tk_before(kb, pb, ka, pa) : tk_before(ka, pa, kb, pb)) {
          const int32_t sa = s_src[i], sb = s_src[j];
          s_key[i] = kb; s_key[j] = ka;
          s_part[i] = pb; s_part[j] = pa;
          s_src[i] = sb; s_src[j] = sa;
        }
        __syncthreads();
      }
    nlist = min(k, nlist + nbuf);
    nbuf = 0;
    changed = true;
    if (nlist == k) { thr_key = s_key[k - 1]; thr_part = s_part[k - 1]; }
  };

  for (int q0 = 0; q0 < T; q0 += TK_THREADS) {
    const int q = q0 + tid;
    unsigned long long key = 0ull;
    int32_t partner = 0, src = 0;
    bool valid = q < T;
    if (valid) {
      long long p;
      if (q < n_col) {
        const int i = row_a + q;
        partner = i;
        p = tk_rowoff(S, i) - base + (c - i - 1);
      } else {
        const int j = c + 1 + (q - n_col);
        partner = j;
        p = row_c + (j - c - 1);
      }
      src = (int32_t)p;
      const double raw = out4[4 * p];
      valid = raw == raw;   // an NA pair is no one's partner
      key = tk_sortable(raw);
    }
    bool surv = valid && (nlist < k || tk_before(key, partner, thr_key, thr_part));
    unsigned long long ballot = __ballot(surv);
    if (lane == 0) s_wcnt[par][wave] = __popcll(ballot);
    __syncthreads();
    int w0 = s_wcnt[par][0], w1 = s_wcnt[par][1], w2 = s_wcnt[par][2], w3 = s_wcnt[par][3];
    int total = w0 + w1 + w2 + w3;
    par ^= 1;
    if (total == 0) continue;
    if (nbuf + total > TK_CAP) {
      flush();   // the buffer is empty afterwards and the threshold has risen: fewer of this pass's candidates survive
      surv = valid && (nlist < k || tk_before(key, partner, thr_key, thr_part));
      ballot = __ballot(surv);
      if (lane == 0) s_wcnt[par][wave] = __popcll(ballot);
      __syncthreads();
      w0 = s_wcnt[par][0]; w1 = s_wcnt[par][1]; w2 = s_wcnt[par][2]; w3 = s_wcnt[par][3];
      total = w0 + w1 + w2 + w3;
      par ^= 1;
    }
    if (surv) {
      const int before_me = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0) +
                            __popcll(ballot & ((1ull << lane) - 1ull));
      const int at = TK_CAP + nbuf + before_me;   // < 2 TK_CAP: nbuf + total <= TK_CAP
      s_key[at] = key;
      s_part[at] = partner;
      s_src[at] = src;
    }
    nbuf += total;
  }
  if (nbuf > 0) flush();
  if (!changed) return;
  // the merged list, with its payloads, into the other buffer
  const size_t new_at = ((size_t)(cur ^ 1) * (size_t)S + (size_t)c) * (size_t)k;
  if (tid < nlist) {
    const int32_t src = s_src[tid];
    const double* from = src >= 0 ? out4 + 4 * (size_t)src : L.vals + 4 * (old_at + (size_t)(~src));
    const double v0 = from[0], v1 = from[1], v2 = from[2], v3 = from[3];
    L.key[new_at + tid] = s_key[tid];
    L.partner[new_at + tid] = s_part[tid];
    double* to = L.vals + 4 * (new_at + tid);
    to[0] = v0; to[1] = v1; to[2] = v2; to[3] = v3;
  }
  if (tid == 0) {
    L.count[c] = nlist;
    L.cur[c] = cur ^ 1;
  }
}

// idx [S][k], out5k [5][S][k] (cor, raw, pvalue, taumax, completeness), n_valid [S]; slots beyond a column's list: -1
// and R's NA_real_.  cor is k_assemble's expression on k_assemble's operands.
__global__ void __launch_bounds__(256)
k_topk_finish(TopkLists L, const unsigned long long* __restrict__ red, int S, int scale_max, int32_t* __restrict__ idx,
              double* __restrict__ out5k, int32_t* __restrict__ n_valid) {
  const long long k = L.k, SK = (long long)S * k;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= SK) return;
  const int c = (int)(t / k), s = (int)(t % k);
  const int cnt = L.count[c];
  if (s == 0 && n_valid) n_valid[c] = cnt;
  if (s < cnt) {
    const size_t at = ((size_t)L.cur[c] * (size_t)S + (size_t)c) * (size_t)k + (size_t)s;
    const double raw = L.vals[4 * at + 0], pval = L.vals[4 * at + 1], tmax = L.vals[4 * at + 2], comp = L.vals[4 * at + 3];
    // max(numeric(0), na.rm = TRUE) is -Inf in R
    const double max_cor = red[0] ? tk_unsortable(red[0]) : -__longlong_as_double(0x7FF0000000000000ll);
    const double cor = scale_max ? raw / max_cor : raw;
    idx[t] = L.partner[at];
    out5k[t] = cor;
    out5k[SK + t] = raw;
    out5k[2 * SK + t] = pval;
    out5k[3 * SK + t] = tmax;
    out5k[4 * SK + t] = comp;
  } else {
    const double NA = __longlong_as_double(0x7FF00000000007A2ll);  // R's NA_real_
    idx[t] = -1;
    out5k[t] = NA;
    out5k[SK + t] = NA;
    out5k[2 * SK + t] = NA;
    out5k[3 * SK + t] = NA;
    out5k[4 * SK + t] = NA;
  }
}

}  // namespace

hipError_t launch_topk_merge(const TopkLists& L, const double* out4, int S, int row_a, int row_b, hipStream_t s) {
  if (row_a < 0 || row_b <= row_a || row_b > S - 1 || L.k < 1 || L.k > TK_CAP) return hipErrorInvalidValue;
  (void)hipGetLastError();
  const long long base = (long long)row_a * (2ll * S - row_a - 1) / 2;
  hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)(S - row_a)), dim3(TK_THREADS), 0, s, L, out4, S, row_a, row_b, base);
  return hipGetLastError();
}

hipError_t launch_topk_finish(const TopkLists& L, const unsigned long long* red, int S, int scale_max, int32_t* idx,
                              double* out5k, int32_t* n_valid, hipStream_t s) {
  const long long SK = (long long)S * L.k;
  if (SK <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_topk_finish, dim3((unsigned)((SK + 255) / 256)), dim3(256), 0, s, L, red, S, scale_max, idx, out5k,
                     n_valid);
  return hipGetLastError();
}

}  // namespace icikt
