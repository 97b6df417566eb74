// icikt_sparse.hip -- a compressed-sparse-column matrix as the library's: float64, column-major.
// k_scatter_csc<T, I> writes nc columns of the column-major float64 device matrix from a DEVICE block that holds a
// chunk's values (element type T: float64, float32, int32, int64) and row indices (I: int32, int64); the column offsets
// (indptr, the whole array, on the device) are rebased to the block by `base`.  A column is ONE workgroup's: it clears
// an LDS bitset of n bits, writes `fill` to rows [0, n) with coalesced 8-byte stores, passes a barrier, and scatters the
// column's entries -- the barrier (a workgroup-scope release / acquire pair around s_barrier) orders the fill store of a
// cell before the entry's store to the same cell, whichever threads issue them.  An entry whose row lies outside [0, n),
// a second entry of a row (atomicOr on the bitset: the old bit tells the second writer) and a column whose offsets do
// not lie inside the block are REJECTED: nothing is stored through them, and the first rejection of a launch is recorded
// in `err` (kind, column, position, row) for the host to report.  The conversion is k_ingest's: (double)v, a float64
// cell as 64 bits.  Memory-bound: it writes 8 * n * nc bytes once and reads nnz * (sizeof T + sizeof I).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icikt.h"
#include "icikt_device.h"

namespace icikt {
namespace {

constexpr int ST = 256;          // threads per workgroup
constexpr int SGRID_CAP = 1024;  // workgroups of a launch, whatever the matrix: four per CU (at 262 144 rows the bitset
                                 // is 32 KB: five workgroups fit a CU's 160 KB); further columns take a later round

template <typename T>
__device__ __forceinline__ unsigned long long widen_s(T v) {
  return (unsigned long long)__double_as_longlong((double)v);
}
template <>
__device__ __forceinline__ unsigned long long widen_s<unsigned long long>(unsigned long long v) { return v; }   // float64: the bits

__device__ __forceinline__ void reject(unsigned long long* err, unsigned long long kind, long long col, long long pos,
                                       long long row) {
  if (atomicCAS(err, 0ull, kind) == 0ull) {   // the first rejection of the launch (which one that is: unspecified)
    err[1] = (unsigned long long)col;
    err[2] = (unsigned long long)pos;
    err[3] = (unsigned long long)row;
  }
}

// vals / idx: the block (entry e of the matrix at vals[e - base]); indptr[col0 + j .. col0 + j + 1]: column j's entries;
// block_nnz: entries the block holds; dst: column j at dst + j * dst_ld, rows [n, dst_ld) not written.
template <typename T, typename I>
__global__ __launch_bounds__(ST) void k_scatter_csc(const T* __restrict__ vals, const I* __restrict__ idx,
                                                    const I* __restrict__ indptr, long long col0, long long base,
                                                    long long block_nnz, unsigned long long fill, long long n,
                                                    long long nc, unsigned long long* __restrict__ dst, long long dst_ld,
                                                    unsigned long long* __restrict__ err) {
  extern __shared__ unsigned int seen[];   // n bits
  const int words = (int)((n + 31) >> 5);
  for (long long j = blockIdx.x; j < nc; j += gridDim.x) {
    unsigned long long* d = dst + j * dst_ld;
    for (int w = threadIdx.x; w < words; w += ST) seen[w] = 0u;
    for (long long r = threadIdx.x; r < n; r += ST) d[r] = fill;
    const long long p0 = (long long)indptr[col0 + j] - base, p1 = (long long)indptr[col0 + j + 1] - base;
    __syncthreads();   // the column holds `fill` and the bitset is clear before any entry lands
    if (p0 < 0 || p1 < p0 || p1 > block_nnz) {
      if (threadIdx.x == 0) reject(err, ICIKT_CSC_BAD_INDPTR, col0 + j, p0 + base, 0);
    } else {
      for (long long e = p0 + threadIdx.x; e < p1; e += ST) {
        const long long r = (long long)idx[e];
        if ((unsigned long long)r >= (unsigned long long)n) { reject(err, ICIKT_CSC_BAD_ROW, col0 + j, e + base, r); continue; }
        const unsigned int bit = 1u << (r & 31);
        if (atomicOr(&seen[r >> 5], bit) & bit) { reject(err, ICIKT_CSC_DUPLICATE, col0 + j, e + base, r); continue; }
        d[r] = widen_s<T>(vals[e]);
      }
    }
    __syncthreads();   // the bitset is cleared again only when every entry of this column has been looked up
  }
}

template <typename T, typename I>
hipError_t launch_ti(const void* vals, const void* idx, const void* indptr, int64_t col0, int64_t base, int64_t block_nnz,
                     unsigned long long fill, int64_t n, int64_t nc, double* dst, int64_t dst_ld, unsigned long long* err,
                     hipStream_t s) {
  const unsigned grid = (unsigned)std::min<long long>(nc, SGRID_CAP);
  const size_t lds = (size_t)((n + 31) >> 5) * sizeof(unsigned int);   // at most 32 KB (n <= ICIKT_MAX_FEATURES_WIDE)
  (void)hipGetLastError();
  hipLaunchKernelGGL((k_scatter_csc<T, I>), dim3(grid), dim3(ST), lds, s, static_cast<const T*>(vals),
                     static_cast<const I*>(idx), static_cast<const I*>(indptr), (long long)col0, (long long)base,
                     (long long)block_nnz, fill, (long long)n, (long long)nc, reinterpret_cast<unsigned long long*>(dst),
                     (long long)dst_ld, err);
  return hipGetLastError();
}

template <typename I>
hipError_t launch_i(const void* vals, int dtype, const void* idx, const void* indptr, int64_t col0, int64_t base,
                    int64_t block_nnz, unsigned long long fill, int64_t n, int64_t nc, double* dst, int64_t dst_ld,
                    unsigned long long* err, hipStream_t s) {
  switch (dtype) {
    case ICIKT_DTYPE_F64: return launch_ti<unsigned long long, I>(vals, idx, indptr, col0, base, block_nnz, fill, n, nc, dst, dst_ld, err, s);
    case ICIKT_DTYPE_F32: return launch_ti<float, I>(vals, idx, indptr, col0, base, block_nnz, fill, n, nc, dst, dst_ld, err, s);
    case ICIKT_DTYPE_I32: return launch_ti<int, I>(vals, idx, indptr, col0, base, block_nnz, fill, n, nc, dst, dst_ld, err, s);
    case ICIKT_DTYPE_I64: return launch_ti<long long, I>(vals, idx, indptr, col0, base, block_nnz, fill, n, nc, dst, dst_ld, err, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_scatter_csc(const void* vals, int dtype, const void* idx, const void* indptr, int index_type,
                              int64_t col0, int64_t base, int64_t block_nnz, double fill, int64_t n, int64_t nc,
                              double* dst, int64_t dst_ld, unsigned long long* err, hipStream_t s) {
  if (n <= 0 || nc <= 0) return hipSuccess;
  if (n > ICIKT_MAX_FEATURES_WIDE) return hipErrorInvalidValue;   // (the bitset must fit the LDS)
  unsigned long long fb;
  __builtin_memcpy(&fb, &fill, sizeof(fb));
  return index_type == ICIKT_INDEX_I64
             ? launch_i<long long>(vals, dtype, idx, indptr, col0, base, block_nnz, fb, n, nc, dst, dst_ld, err, s)
             : launch_i<int>(vals, dtype, idx, indptr, col0, base, block_nnz, fb, n, nc, dst, dst_ld, err, s);
}

}  // namespace icikt
