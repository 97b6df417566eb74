// icikt_wave.h -- wavefront primitives (wave64, DPP, ds_swizzle, permlane swaps) shared by the device units
// icikt_kernels.hip, icikt_prepass.hip and icikt_epilogue.hip.  Device-only, all inline: include it from a .hip file.
#ifndef ICIKT_WAVE_H
#define ICIKT_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icikt {

// ------------------------------------------------------------------------------------------------
// wavefront primitives (wave64, DPP)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// whole-wave shift right by one lane; lane 0 keeps `old`
__device__ __forceinline__ uint32_t dpp_wave_shr1(uint32_t old, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
}

// inclusive prefix sum over the 64 lanes: row_shr 1/2/4/8 inside each row of 16, then row_bcast 15 / 31
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /*row_bcast:15*/, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /*row_bcast:31*/, 0xc, 0xf, false);
  return v;
}

// Whole-wave reductions as a butterfly over ds_swizzle (lane ^ 1 .. 16: the pattern is an immediate) and
// v_permlane32_swap (lane ^ 32).  (__shfl_xor goes through ds_bpermute with one address register per distance;
// hipcc keeps those five registers alive from the first reduction of a task to the last -- across the hot loop --
// and spills them.  DPP scans need no addresses either, but cost three times the vector instructions.)
template <int X>
__device__ __forceinline__ uint32_t swz_xor(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1F);
}
__device__ __forceinline__ uint32_t xor32(uint32_t v) {
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);   // [0]: lanes 0..31 twice, [1]: lanes 32..63 twice
  return r[0] ^ r[1] ^ v;                                                // the other half's value
}
template <int X>
__device__ __forceinline__ unsigned long long swz_xor64(unsigned long long v) {
  return (unsigned long long)swz_xor<X>((uint32_t)v) | ((unsigned long long)swz_xor<X>((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  v += swz_xor64<1>(v);
  v += swz_xor64<2>(v);
  v += swz_xor64<4>(v);
  v += swz_xor64<8>(v);
  v += swz_xor64<16>(v);
  v += (unsigned long long)xor32((uint32_t)v) | ((unsigned long long)xor32((uint32_t)(v >> 32)) << 32);
  return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
  v = max(v, (int)swz_xor<1>((uint32_t)v));
  v = max(v, (int)swz_xor<2>((uint32_t)v));
  v = max(v, (int)swz_xor<4>((uint32_t)v));
  v = max(v, (int)swz_xor<8>((uint32_t)v));
  v = max(v, (int)swz_xor<16>((uint32_t)v));
  v = max(v, (int)xor32((uint32_t)v));
  return v;
}

// Orders this wave's LDS traffic for the compiler: lanes of one wave exchange data through LDS
// (atomic OR by one lane, read by another).  The hardware keeps one wave's DS operations in order;
// this keeps the compiler from moving accesses across the hand-off.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave-uniform 64-bit value moved to scalar registers (readfirstlane returns a SIGNED int:
// widen through uint32_t, or bit 31 smears into the upper word)
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// global loads addressed as uniform base + 32-bit per-lane offset (saddr form: no 64-bit VALU address math)
__device__ __forceinline__ uint32_t gload_u32(const uint32_t* base, uint32_t idx) {
  return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(base) + (size_t)(idx << 2));
}
__device__ __forceinline__ uint32_t gload_u16(const uint16_t* base, uint32_t idx) {
  return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(base) + (size_t)(idx << 1));
}

// both columns of a rec block for the lane's row: [row][2] u32, one 8-byte gather
__device__ __forceinline__ uint2 gload_rec2(const uint32_t* blk, uint32_t row) {
  return *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(blk) + (size_t)(row << 3));
}

// set bit `pos` of an LDS bitset: a 32-bit LDS atomic on the half of the 64-bit word that holds the bit
// (little endian: word w = dwords 2w, 2w+1), half the data of a 64-bit one
__device__ __forceinline__ void seen_insert(unsigned long long* bits, uint32_t pos) {
  atomicOr(reinterpret_cast<uint32_t*>(bits) + (pos >> 5), 1u << (pos & 31u));
}

// popcount(x) + acc in the one instruction that does both (hipcc splits chains of these into popcounts and adds)
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}
// (hi << 16) | lo in one instruction (hipcc emits a shift and an OR when it can prove the operands disjoint)
__device__ __forceinline__ uint32_t pack16(uint32_t hi, uint32_t lo) {
  uint32_t r;
  asm("v_lshl_or_b32 %0, %1, 16, %2" : "=v"(r) : "v"(hi), "v"(lo));
  return r;
}
__device__ __forceinline__ uint32_t bcnt64_acc(unsigned long long x, uint32_t acc) {
  return bcnt_acc((uint32_t)(x >> 32), bcnt_acc((uint32_t)x, acc));
}
__device__ __forceinline__ unsigned long long low_mask64(uint32_t bits /*0..63*/) {
  return (1ull << bits) - 1ull;
}

// Block-wide reductions (the pre-pass, icikt_prepass.hip): inside a wave by shuffles, across the waves through one small LDS table -- one or two workgroup
// barriers per BATCH of values.  (Rounds 1-3 ran a 1 024-entry LDS tree per value: 12 barriers each, 14 values per
// column: 170 of a column's ~450 barriers.  Removing them changed nothing: the pre-pass is bound by the vector
// instructions of its sort network, see kv_gt.)
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
// value of lane ^ J for J = 1, 2, 4, 8, 16, 32 without LDS: quad_perm for 1 and 2, row_shl / row_shr 4 with a
// select, row_ror:8 (inside a 16-lane row rotating by 8 IS xor 8), v_permlane16_swap / v_permlane32_swap of two
// copies for 16 and 32.  Every DPP runs with all lanes active; the selects come afterwards.
template <int J>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, uint32_t lane) {
  if (J == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /*quad_perm:[1,0,3,2]*/, 0xf, 0xf, false);
  if (J == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /*quad_perm:[2,3,0,1]*/, 0xf, 0xf, false);
  if (J == 4) {
    const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104 /*row_shl:4*/, 0xf, 0xf, false);
    const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /*row_shr:4*/, 0xf, 0xf, false);
    return (lane & 4u) ? dn : up;
  }
  if (J == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /*row_ror:8*/, 0xf, 0xf, false);
  if (J == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // r[0] = rows [0,0,2,2], r[1] = rows [1,1,3,3]
    return (lane & 16u) ? r[0] : r[1];
  }
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);    // r[0] = halves [lo, lo], r[1] = [hi, hi]
  return (lane & 32u) ? r[0] : r[1];
}

}  // namespace icikt
#endif
