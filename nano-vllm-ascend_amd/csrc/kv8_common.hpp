// The fp8 (e4m3) KV cache tile: addressing, the exact dequantisation in registers and the quantisation rule, shared by
// paged_attn_fp8kv.hip (store, decode attention, expansion) and prefill_fp8kv.hip (prefill attention, the prefill-sized
// fused store).  The layout itself is described at the head of paged_attn_fp8kv.hip and in include/mi355_nanovllm.h.
#pragma once
#include "mi_common.hpp"

namespace mi {

constexpr int KV8_DATA = 2048;              // e4m3 bytes of a tile; the scales follow
constexpr int KV8_TILE = MI_KV8_TILE_BYTES;

// byte offset of (t, d) inside a K / V tile
__host__ __device__ __forceinline__ int k8_tile_off(int t, int d) {
  return (d >> 6) * 1024 + ((((d >> 3) & 3) * 16 + t) << 4) + ((d >> 5) & 1) * 8 + (d & 7);
}
__host__ __device__ __forceinline__ int v8_tile_off(int t, int d) {
  return (d >> 6) * 1024 + ((((t >> 2) * 16) + (d & 15)) << 4) + ((d >> 4) & 3) * 4 + (t & 3);
}
__host__ __device__ __forceinline__ int64_t kv8_tile_base(int64_t blk, int h, int slot_in_block, int n_kv_heads, int tpb) {
  return ((blk * n_kv_heads + h) * tpb + (slot_in_block >> 4)) * (int64_t)KV8_TILE;
}

// four e4m3 -> four bf16 (exact: the upper halves of the fp32 conversions)
__device__ __forceinline__ u32x2 dq4(uint32_t w) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  return u32x2{__builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u),
               __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u)};
}
__device__ __forceinline__ bf16x8 dq8(uint32_t w0, uint32_t w1) {
  const u32x2 a = dq4(w0), b = dq4(w1);
  return as_frag(u32x4{a[0], a[1], b[0], b[1]});
}

// The quantisation rule, shared by the store kernels and the fused decode step.  floor(log2 amax) is the exponent field
// (a bf16 subnormal maximum falls under the clamp in any case).
__device__ __forceinline__ int kv8_exponent(float amax) {
  return amax == 0.f ? 0 : max((int)(__float_as_uint(amax) >> 23) - 127 - 7, -120);
}
// four values times 2^-e -> four e4m3 bytes, the first in the low byte
__device__ __forceinline__ uint32_t quant4(float a, float b, float c, float d, float inv) {
  const int w = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, 0, false);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, w, true);
}

inline int check_kv8(int n_kv_heads, int head_dim, int block_size) {
  if (n_kv_heads <= 0) return MI_EINVAL;
  if (head_dim != MI_HEAD_DIM || block_size <= 0 || block_size % 16) return MI_EUNSUPPORTED;
  return MI_OK;
}

}  // namespace mi
