// icikt_ingest.hip -- the caller's matrix as the library's: float64, column-major.
// k_ingest<T, ROW> writes nc columns of the column-major float64 device matrix from a DEVICE block of element type T
// (float64, float32, int32, int64) in column-major (ROW = false) or row-major (ROW = true) layout.  The conversion is
// C's (double)v; a float64 cell travels as 64 bits, so NaN payloads (NA_real_) survive.  Memory-bound: it reads
// n * nc * sizeof(T) and writes 8 * n * nc bytes once, coalesced on both sides.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "icikt.h"
#include "icikt_device.h"

namespace icikt {
namespace {

constexpr int IT = 256;      // threads per workgroup
constexpr int TILE = 64;     // ROW: a tile is TILE features x TILE samples
constexpr int TILE_LD = 65;  // its LDS row in 8-byte words.  Filled row by row (ds_write_b64, 16 contiguous lanes =
                             // 32 banks), read column by column (ds_read_b64, bank (a / 4) mod 64, 32-lane groups):
                             // lane x reads dwords 130 x + 2 cc, 130 x mod 64 = 2 x: 32 lanes, 32 distinct even banks.
                             // An unpadded row (64 words) would put all 32 lanes of the read on one bank pair.
constexpr int COL_ROWS = 512;   // COL: a tile is COL_ROWS rows of one column
constexpr int GRID_CAP = 1024;  // workgroups of a launch, whatever the matrix: four per CU, what the ROW tile's 33 KB of
                                // LDS leave room for (the tiles beyond take a later round of the grid-stride loop)

template <typename T>
__device__ __forceinline__ unsigned long long widen(T v) {
  return (unsigned long long)__double_as_longlong((double)v);
}
template <>
__device__ __forceinline__ unsigned long long widen<unsigned long long>(unsigned long long v) { return v; }   // float64: the bits

// src: element (r, c) at src[r + c * src_ld] (COL) or src[r * src_ld + c] (ROW); dst: column c at dst + c * dst_ld.
// Rows [n, dst_ld) of dst are not written.
template <typename T, bool ROW>
__global__ __launch_bounds__(IT) void k_ingest(const T* __restrict__ src, long long src_ld, long long n, long long nc,
                                               unsigned long long* __restrict__ dst, long long dst_ld, long long tiles_r,
                                               long long n_tiles) {
  if constexpr (ROW) {
    __shared__ unsigned long long tile[TILE * TILE_LD];
    const int x = (int)(threadIdx.x & (TILE - 1)), y = (int)(threadIdx.x / TILE);   // y: 0 .. 3
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
      const long long r0 = (t % tiles_r) * TILE, c0 = (t / tiles_r) * TILE;
      // rows of the source, coalesced along the sample index
      if (c0 + x < nc)
        for (int k = y; k < TILE && r0 + k < n; k += IT / TILE)
          tile[k * TILE_LD + x] = widen<T>(src[(r0 + k) * src_ld + (c0 + x)]);
      __syncthreads();
      // columns of the destination, coalesced along the feature index
      if (r0 + x < n)
        for (int k = y; k < TILE && c0 + k < nc; k += IT / TILE)
          dst[(c0 + k) * dst_ld + (r0 + x)] = tile[x * TILE_LD + k];
      __syncthreads();
    }
  } else {
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
      const long long r0 = (t % tiles_r) * COL_ROWS, c = t / tiles_r;
      const T* s = src + c * src_ld;
      unsigned long long* d = dst + c * dst_ld;
#pragma unroll
      for (int k = 0; k < COL_ROWS / IT; ++k) {
        const long long r = r0 + k * IT + threadIdx.x;
        if (r < n) d[r] = widen<T>(s[r]);
      }
    }
  }
}

template <typename T, bool ROW>
hipError_t launch_t(const void* src, int64_t src_ld, int64_t n, int64_t nc, double* dst, int64_t dst_ld, hipStream_t s) {
  const long long tiles_r = ROW ? (n + TILE - 1) / TILE : (n + COL_ROWS - 1) / COL_ROWS;
  const long long n_tiles = tiles_r * (ROW ? (nc + TILE - 1) / TILE : nc);
  const unsigned grid = (unsigned)std::min<long long>(n_tiles, GRID_CAP);
  (void)hipGetLastError();
  hipLaunchKernelGGL((k_ingest<T, ROW>), dim3(grid), dim3(IT), 0, s, static_cast<const T*>(src), (long long)src_ld,
                     (long long)n, (long long)nc, reinterpret_cast<unsigned long long*>(dst), (long long)dst_ld, tiles_r,
                     n_tiles);
  return hipGetLastError();
}

template <bool ROW>
hipError_t launch_o(const void* src, int dtype, int64_t src_ld, int64_t n, int64_t nc, double* dst, int64_t dst_ld,
                    hipStream_t s) {
  switch (dtype) {
    case ICIKT_DTYPE_F64: return launch_t<unsigned long long, ROW>(src, src_ld, n, nc, dst, dst_ld, s);
    case ICIKT_DTYPE_F32: return launch_t<float, ROW>(src, src_ld, n, nc, dst, dst_ld, s);
    case ICIKT_DTYPE_I32: return launch_t<int, ROW>(src, src_ld, n, nc, dst, dst_ld, s);
    case ICIKT_DTYPE_I64: return launch_t<long long, ROW>(src, src_ld, n, nc, dst, dst_ld, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_ingest(const void* src, int dtype, int order, int64_t src_ld, int64_t n, int64_t nc, double* dst,
                         int64_t dst_ld, hipStream_t s) {
  if (n <= 0 || nc <= 0) return hipSuccess;
  return order == ICIKT_ORDER_ROW ? launch_o<true>(src, dtype, src_ld, n, nc, dst, dst_ld, s)
                                  : launch_o<false>(src, dtype, src_ld, n, nc, dst, dst_ld, s);
}

}  // namespace icikt
