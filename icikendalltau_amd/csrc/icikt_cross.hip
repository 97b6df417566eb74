// icikt_cross.hip -- the folds of the query x reference rectangle (icikt_cross_f64, icikt_ref_cross_f64; host side:
// icikt_capi_cross.cpp).
//
// The pair engine runs the rectangle in blocks of whole query rows; a block's out4 records are query-major, so the Sr
// records of a query lie one behind the other and are all there.  k_cross_topk therefore selects a query's k best
// reference columns in ONE pass over its row and writes the final lists: no list survives a block, nothing is merged
// at the end.  k_cross_planes turns a block's records into the four value planes at the block's place.  cor needs the
// largest taumax of the whole rectangle (word 0 of d_red), which is final only behind the last block: k_cross_cor
// fills that plane then.  With class labels on the reference, k_cross_class finds the two middle raw of every (query,
// class) cell inside the row's own block -- a radix select over the class's records of the row (icikt_select.h) -- and
// k_cross_class_cor turns them into the medians behind the last block.  No kernel here waits for another workgroup, and none uses a global atomic.
//
// The order of a list is icikt_topk.hip's, STRICT: raw descending in the total order of the sortable key (-0.0 below
// +0.0), ties by the smaller reference index.  The threshold test, the compaction and the sort all go through
// cx_before(), so a query's list is a pure function of its row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icikt_colsort.h"
#include "icikt_device.h"
#include "icikt_select.h"

namespace icikt {

namespace {

constexpr int CX_THREADS = 256;        // one workgroup (4 waves) per query row
constexpr int CX_CAP = 256;            // == ICIKT_TOPK_MAX: entries of a list, and of the survivor buffer behind it
constexpr int CX_SENTINEL = 0x7FFFFFFF;

// monotone in v; 0 is below every double (dbl_sortable of icikt_epilogue.hip, tk_sortable of icikt_topk.hip)
__device__ __forceinline__ unsigned long long cx_sortable(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double cx_unsortable(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
// the list's strict order: does (ka, ra) come before (kb, rb)?
__device__ __forceinline__ bool cx_before(unsigned long long ka, int32_t ra, unsigned long long kb, int32_t rb) {
  return ka > kb || (ka == kb && ra < rb);
}
__device__ __forceinline__ double cx_na() { return __longlong_as_double(0x7FF00000000007A2ll); }   // R's NA_real_

// One workgroup per query row q = row_first + blockIdx.x of the block; its candidates are the records
// out4[(blockIdx.x * Sr + r) * 4 ..], r in [0, Sr).  LDS: entries [0, 256) the list (sorted, nlist of them), [256, 512)
// the survivors that beat the list's k-th entry, as two arrays (8-byte keys, 4-byte reference indices): a reference
// index is also the place of its record in the row, so the payload needs no word of its own.
// idx [Sq][k], planes [5][Sq][k] (plane 0, cor, is k_cross_cor's), n_valid [Sq]: the row's k slots are all written.
__global__ void __launch_bounds__(CX_THREADS)
k_cross_topk(const double* __restrict__ out4, int Sr, int k, int row_first, long long SK, int32_t* __restrict__ idx,
             double* __restrict__ planes, int32_t* __restrict__ n_valid) {
  __shared__ unsigned long long s_key[2 * CX_CAP];
  __shared__ int32_t s_ref[2 * CX_CAP];
  __shared__ int s_wcnt[2][CX_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ row = out4 + 4 * (size_t)blockIdx.x * (size_t)Sr;
  int nlist = 0, nbuf = 0, par = 0;
  unsigned long long thr_key = 0ull;
  int32_t thr_ref = CX_SENTINEL;

  // list U buffer -> the first min(k, nlist + nbuf) of their union in the list's order.  Every thread runs it with the
  // same nlist / nbuf (registers, derived from workgroup-uniform values only).
  auto flush = [&]() {
    __syncthreads();   // the buffer's entries are written
    for (int i = tid; i < 2 * CX_CAP; i += CX_THREADS)
      if ((i >= nlist && i < CX_CAP) || i >= CX_CAP + nbuf) {
        s_key[i] = 0ull;   // below every candidate: NaN is dropped before it gets a key
        s_ref[i] = CX_SENTINEL;
      }
    __syncthreads();
    for (int size = 2; size <= 2 * CX_CAP; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        const int i = ((tid & ~(stride - 1)) << 1) | (tid & (stride - 1)), j = i + stride;
        const unsigned long long ka = s_key[i], kb = s_key[j];
        const int32_t ra = s_ref[i], rb = s_ref[j];
        const bool fwd = (i & size) == 0;   // this run ends in the list's order (else in its reverse)
        if (fwd ? cx_before(kb, rb, ka, ra) : cx_before(ka, ra, kb, rb)) {
          s_key[i] = kb; s_key[j] = ka;
          s_ref[i] = rb; s_ref[j] = ra;
        }
        __syncthreads();
      }
    nlist = min(k, nlist + nbuf);
    nbuf = 0;
    if (nlist == k) { thr_key = s_key[k - 1]; thr_ref = s_ref[k - 1]; }
  };

  for (int r0 = 0; r0 < Sr; r0 += CX_THREADS) {
    const int r = r0 + tid;
    unsigned long long key = 0ull;
    bool valid = r < Sr;
    if (valid) {
      const double raw = row[4 * (size_t)r];
      valid = raw == raw;   // an NA pair is no partner
      key = cx_sortable(raw);
    }
    bool surv = valid && (nlist < k || cx_before(key, r, thr_key, thr_ref));
    unsigned long long ballot = __ballot(surv);
    if (lane == 0) s_wcnt[par][wave] = __popcll(ballot);
    __syncthreads();
    int w0 = s_wcnt[par][0], w1 = s_wcnt[par][1], w2 = s_wcnt[par][2], w3 = s_wcnt[par][3];
    int total = w0 + w1 + w2 + w3;
    par ^= 1;
    if (total == 0) continue;
    if (nbuf + total > CX_CAP) {
      flush();   // the buffer is empty afterwards and the threshold has risen: fewer of this pass's candidates survive
      surv = valid && (nlist < k || cx_before(key, r, thr_key, thr_ref));
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
      const int at = CX_CAP + nbuf + before_me;   // < 2 CX_CAP: nbuf + total <= CX_CAP
      s_key[at] = key;
      s_ref[at] = r;
    }
    nbuf += total;
  }
  if (nbuf > 0) flush();   // (ends on a barrier: the list is readable)

  const long long q = (long long)row_first + blockIdx.x;
  if (tid < k) {
    const long long t = q * k + tid;
    if (tid < nlist) {
      const int32_t r = s_ref[tid];
      const double* __restrict__ rec = row + 4 * (size_t)r;
      const double v0 = rec[0], v1 = rec[1], v2 = rec[2], v3 = rec[3];
      idx[t] = r;
      planes[SK + t] = v0;
      planes[2 * SK + t] = v1;
      planes[3 * SK + t] = v2;
      planes[4 * SK + t] = v3;
    } else {
      const double NA = cx_na();
      idx[t] = -1;
      planes[SK + t] = NA;
      planes[2 * SK + t] = NA;
      planes[3 * SK + t] = NA;
      planes[4 * SK + t] = NA;
    }
  }
  if (tid == 0) n_valid[q] = nlist;
}

// a block's records [count][4] -> planes 1 .. 4 (raw, pvalue, taumax, completeness) of planes [5][P] at [begin, begin +
// count): a thread per pair, its record one 32-byte read, every plane's stores one behind the other
__global__ void __launch_bounds__(256)
k_cross_planes(const double* __restrict__ out4, long long count, long long begin, long long P, double* __restrict__ planes) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  const double2* __restrict__ rec = reinterpret_cast<const double2*>(out4) + 2 * (size_t)p;
  const double2 a = rec[0], b = rec[1];
  const long long t = begin + p;
  planes[P + t] = a.x;
  planes[2 * P + t] = a.y;
  planes[3 * P + t] = b.x;
  planes[4 * P + t] = b.y;
}

// plane 0 of planes [5][P] from plane 1 once red is final: k_assemble's expression on k_assemble's operands; idx (may
// be null): a slot with idx < 0 is padding, NA_real_
__global__ void __launch_bounds__(256)
k_cross_cor(const unsigned long long* __restrict__ red, int scale_max, const int32_t* __restrict__ idx, long long P,
            double* __restrict__ planes) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P) return;
  if (idx && idx[t] < 0) {
    planes[t] = cx_na();
    return;
  }
  const double raw = planes[P + t];
  // max(numeric(0), na.rm = TRUE) is -Inf in R
  const double max_cor = red[0] ? cx_unsortable(red[0]) : -__longlong_as_double(0x7FF0000000000000ll);
  planes[t] = scale_max ? raw / max_cor : raw;
}

// column `col` of the column-major n-row matrix dX: every cell NaN, a missing value under every exclusion rule
__global__ void __launch_bounds__(256)
k_cross_pad(double* __restrict__ col, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) col[t] = __longlong_as_double(0x7FF8000000000000ll);
}

// The class fold (icikt_ref_cross_*: a labelled reference).  One workgroup per cell (query row blockIdx.x of the block,
// class blockIdx.y).  Class c is member[first[c] .. first[c + 1]), reference columns; key t of the cell is the raw of the
// row's record of member[first[c] + t] as a sortable key (colsort::cor_key: NA_KEY for an NA pair, a zero as +0).  The
// row's records are all in this block, so the cell is final here: cells [2][C][Sq] takes its lower and its upper middle
// KEY (k_cross_class_cor turns them into values once the scale is known), n_valid [C][Sq] its partners.  stage: keys the
// LDS buffer takes (<= MEDIAN_STAGE_MAX); a larger cell re-reads the member list and the records in every pass.
__global__ void __launch_bounds__(colsort::CT)
k_cross_class(const double* __restrict__ out4, const int32_t* __restrict__ member, const int32_t* __restrict__ first, int Sr,
              int n_class, int row_first, long long Sq, int stage, unsigned long long* __restrict__ cells,
              int32_t* __restrict__ n_valid) {
  __shared__ unsigned long long s_keys[MEDIAN_STAGE_MAX];
  __shared__ sel::Scratch s_sel;
  const int tid = threadIdx.x;
  const int c = (int)blockIdx.y;
  if (c >= n_class) return;
  const double* __restrict__ row = out4 + 4 * (size_t)blockIdx.x * (size_t)Sr;
  const int f0 = first[c];
  const int T = first[c + 1] - f0;
  const bool staged = T <= stage;
  auto load = [&](int t) -> unsigned long long { return colsort::cor_key(row[4 * (size_t)member[f0 + t]]); };
  if (staged)
    for (int t = tid; t < T; t += colsort::CT) s_keys[t] = load(t);
  __syncthreads();
  auto key_at = [&](int t) -> unsigned long long { return staged ? s_keys[t] : load(t); };

  unsigned long long lower = 0ull, upper = 0ull;
  const int v = sel::middle_keys(T, key_at, s_sel, &lower, &upper);
  if (tid != 0) return;
  const size_t plane = (size_t)Sq * (size_t)n_class, cell = (size_t)c * (size_t)Sq + (size_t)row_first + blockIdx.x;
  cells[cell] = v ? lower : 0ull;
  cells[plane + cell] = v ? upper : 0ull;
  n_valid[cell] = v;
}

// cells [2][n_cells]: the middle keys k_cross_class left -> (med_cor, med_raw) in their place, once red is final; a
// cell without a partner is NA_real_.  The values are sel::median_values', as in k_class_select.
__global__ void __launch_bounds__(256)
k_cross_class_cor(const unsigned long long* __restrict__ red, int scale_max, const int32_t* __restrict__ n_valid,
                  long long n_cells, unsigned long long* cells) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_cells) return;
  const int v = n_valid[t];
  double med_cor = cx_na(), med_raw = cx_na();
  if (v > 0) sel::median_values(cells[t], cells[n_cells + t], v, red[0], scale_max, &med_cor, &med_raw);
  cells[t] = (unsigned long long)__double_as_longlong(med_cor);
  cells[n_cells + t] = (unsigned long long)__double_as_longlong(med_raw);
}

}  // namespace

hipError_t launch_cross_class(const double* out4, const int32_t* member, const int32_t* first, int Sr, int n_class,
                              int row_first, int n_rows, long long Sq, int stage, double* med2, int32_t* n_valid,
                              hipStream_t s) {
  if (Sr < 1 || n_class < 1 || n_class > CLASS_MATRIX_MAX_CLASSES || row_first < 0 || n_rows < 1 ||
      (long long)row_first + n_rows > Sq || stage < 0 || stage > MEDIAN_STAGE_MAX)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cross_class, dim3((unsigned)n_rows, (unsigned)n_class), dim3(colsort::CT), 0, s, out4, member, first,
                     Sr, n_class, row_first, Sq, stage, reinterpret_cast<unsigned long long*>(med2), n_valid);
  return hipGetLastError();
}

hipError_t launch_cross_class_cor(const unsigned long long* red, int scale_max, const int32_t* n_valid, long long n_cells,
                                  double* med2, hipStream_t s) {
  if (n_cells <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cross_class_cor, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, s, red, scale_max, n_valid,
                     n_cells, reinterpret_cast<unsigned long long*>(med2));
  return hipGetLastError();
}

hipError_t launch_cross_topk(const double* out4, int Sr, int k, int row_first, int n_rows, long long Sq, int32_t* idx,
                             double* planes, int32_t* n_valid, hipStream_t s) {
  if (Sr < 1 || k < 1 || k > CX_CAP || row_first < 0 || n_rows < 1 || (long long)row_first + n_rows > Sq) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cross_topk, dim3((unsigned)n_rows), dim3(CX_THREADS), 0, s, out4, Sr, k, row_first, Sq * k, idx,
                     planes, n_valid);
  return hipGetLastError();
}

hipError_t launch_cross_planes(const double* out4, long long count, long long begin, long long P, double* planes,
                               hipStream_t s) {
  if (count <= 0) return hipSuccess;
  if (begin < 0 || begin + count > P) return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cross_planes, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, out4, count, begin, P, planes);
  return hipGetLastError();
}

hipError_t launch_cross_cor(const unsigned long long* red, int scale_max, const int32_t* idx, long long P, double* planes,
                            hipStream_t s) {
  if (P <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cross_cor, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, red, scale_max, idx, P, planes);
  return hipGetLastError();
}

hipError_t launch_cross_pad(double* col, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_cross_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, col, n);
  return hipGetLastError();
}

}  // namespace icikt
