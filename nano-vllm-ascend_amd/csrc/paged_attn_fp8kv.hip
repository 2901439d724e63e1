// Opt-in fp8 (OCP e4m3) paged KV cache for gfx950: store, decode attention, expansion for prefill, gather.
//
// Quantisation (fixed, so that tests are exact): one power-of-two scale per (token, kv head) row of 128 values,
//   amax = max|x|, e = max(floor(log2 amax) - 7, -120) (e = 0 for an all-zero row), scale = 2^e, q = RNE_e4m3fn(x / scale):
// the row maximum lands in [128, 256) of e4m3's +-448; x / scale and q * scale are exact (e4m3's 3 mantissa bits fit
// bf16's 7), so attention over this cache IS attention over the dequantised bf16 rows - the accuracy contract of the
// bf16 kernel carries over unchanged.
//
// Cache layout (include/mi355_nanovllm.h): one tile of MI_KV8_TILE_BYTES = 2048 + 64 bytes per (16 slots, kv head):
//   bytes [0, 2048)     the 16 x 128 e4m3 values as TWO 1 KiB wave loads of 16 B per lane.  Lane (g, n) = (lane / 16,
//                       lane % 16) of load i holds
//                         K: K[token n][64 i + 8 g + e] in bytes 0..7 and K[token n][64 i + 32 + 8 g + e] in bytes 8..15
//                            - after dequantisation two A operands (k-steps 2 i and 2 i + 1) of v_mfma_f32_16x16x32_bf16
//                            for S^T = K . Q^T, tokens on M;
//                         V: dword w = V[tokens 4 g .. 4 g + 3][64 i + 16 w + n] - after dequantisation one half (one
//                            tile's four tokens) of the A operand of O^T[16 (4 i + w) ..] += V^T . P; the other half is
//                            the same dword of the chunk's second tile.  The contraction slot of lane (g, .) is then
//                            (tile 0 tokens 4 g .. 4 g + 3, tile 1 tokens 4 g .. 4 g + 3): the order of the score
//                            registers, so P never moves between lanes.
//   bytes [2048, 2112)  the 16 fp32 scales of the tile's tokens: they arrive with the tile (one 16-byte broadcast load
//                       of tokens 4 g .. 4 g + 3 per lane, address known with the tile's - nothing hangs behind the
//                       block-table lookup but the tile itself), and consecutive tiles of a block stay contiguous.
// The scales cost no MFMA work: K's multiplies the token's fp32 score, V's the token's probability before the bf16
// hi + lo split; both are exact (powers of two).
//
// Decode geometry: the work split of the bf16 kernel (one workgroup per (sequence, kv head[, split]), contiguous runs of
// tiles per wave, per-wave online softmax, LDS merge, fp32 partials + merge kernel for split sequences, ranges derived
// on the device).  A 32-token chunk is 8 KiB + 256 B (12 loads); 8 waves with two chunks in flight each keep 16 KiB
// per wave outstanding in 48 raw VGPRs per chunk (DESIGN.md section 3 says why not deeper).
#include <limits.h>

#include "mi_common.hpp"
#include "kv_store.hpp"
#include "kv8_common.hpp"
#include "prefill_common.hpp"
#include "step_prologue.hpp"

namespace mi {

// (the tile's addressing, dq4 / dq8, the quantisation rule and check_kv8: kv8_common.hpp, shared with the prefill
// kernels of prefill_fp8kv.hip)
typedef __attribute__((ext_vector_type(2))) float f32x2;

// ---------------------------------------------------------------------------
// store: 8 lanes per (token, kv head, K | V) row, 16 values each (dims 8 j .. and 64 + 8 j ..)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                           int64_t k_stride, int64_t v_stride, uint8_t* __restrict__ kc,
                                                           uint8_t* __restrict__ vc, const int32_t* __restrict__ slots,
                                                           int slot_is_2d, int n_tokens, int n_kv_heads, int block_size) {
  const int64_t total = (int64_t)n_tokens * n_kv_heads * 2;
  const int64_t row_raw = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const bool live = row_raw < total;  // (no early return: the DPP reduction needs every lane of the wave)
  const int64_t row = live ? row_raw : 0;
  const int j = threadIdx.x & 7, is_v = (int)(row & 1), h = (int)((row >> 1) % n_kv_heads);
  const int token = (int)((row >> 1) / n_kv_heads);
  const uint16_t* src = (is_v ? v + (int64_t)token * v_stride : k + (int64_t)token * k_stride) + h * 128;
  float a[8], b[8];
  load16(src + 8 * j, a);
  load16(src + 64 + 8 * j, b);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fmaxf(fabsf(a[i]), fabsf(b[i])));
  amax = xor_max<1>(amax);
  amax = xor_max<2>(amax);
  amax = xor_max<4>(amax);
  const int e = kv8_exponent(amax);
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23), scale = __uint_as_float((uint32_t)(127 + e) << 23);
  uint32_t qa[2], qb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    qa[i] = quant4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], inv);
    qb[i] = quant4(b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3], inv);
  }
  int64_t blk;
  int off;
  if (!live || !resolve_slot(slots, slot_is_2d, token, block_size, blk, off)) return;
  uint8_t* tile = (is_v ? vc : kc) + kv8_tile_base(blk, h, off, n_kv_heads, block_size >> 4);
  const int t = off & 15;
  if (!is_v) {  // 8 consecutive dims of a token are 8 consecutive bytes
    *reinterpret_cast<u32x2*>(tile + k8_tile_off(t, 8 * j)) = u32x2{qa[0], qa[1]};
    *reinterpret_cast<u32x2*>(tile + k8_tile_off(t, 64 + 8 * j)) = u32x2{qb[0], qb[1]};
  } else {  // token-transposed: one byte per dim
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      tile[v8_tile_off(t, 8 * j + i)] = (uint8_t)(qa[i >> 2] >> (8 * (i & 3)));
      tile[v8_tile_off(t, 64 + 8 * j + i)] = (uint8_t)(qb[i >> 2] >> (8 * (i & 3)));
    }
  }
  if (j == 0) *reinterpret_cast<float*>(tile + KV8_DATA + 4 * t) = scale;
}

// inverse of the store, for content checks: logical rows of e4m3 bytes and their scales
__global__ __launch_bounds__(256) void kv_gather_fp8_kernel(const uint8_t* __restrict__ cache, int is_v,
                                                            const int32_t* __restrict__ slot_flat, int n,
                                                            uint8_t* __restrict__ out_q, float* __restrict__ out_scale,
                                                            int n_kv_heads, int block_size) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * n_kv_heads * 128) return;
  const int d = (int)(idx & 127), h = (int)((idx >> 7) % n_kv_heads), i = (int)(idx / (128 * (int64_t)n_kv_heads));
  const int32_t s = slot_flat[i];
  if (s < 0) {
    out_q[idx] = 0;
    if (d == 0) out_scale[idx >> 7] = 0.f;
    return;
  }
  const int off = s % block_size;
  const uint8_t* tile = cache + kv8_tile_base(s / block_size, h, off, n_kv_heads, block_size >> 4);
  out_q[idx] = tile[is_v ? v8_tile_off(off & 15, d) : k8_tile_off(off & 15, d)];
  if (d == 0) out_scale[idx >> 7] = *reinterpret_cast<const float*>(tile + KV8_DATA + 4 * (off & 15));
}

// ---------------------------------------------------------------------------
// expand (prefill): grid (blocks per sequence, kv heads, sequences), 4 waves; a wave dequantises whole tiles of the
// blocks the step's tables reference into the bf16 fragment-native scratch AT THE SAME BLOCK ID.  A loaded 16-byte
// quad is two bf16 fragments of the same lane (K and V alike: fp8 load i -> bf16 fragments 2 i and 2 i + 1), so the
// kernel is 1 KiB loads in, 1 KiB stores out, no exchange.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_fp8_expand_kernel(const uint8_t* __restrict__ k8, const uint8_t* __restrict__ v8,
                                                            uint16_t* __restrict__ ks, uint16_t* __restrict__ vs,
                                                            const int32_t* __restrict__ block_table, int table_stride,
                                                            const int32_t* __restrict__ kv_lens, int n_kv_heads, int tpb) {
  const int bi = blockIdx.x, h = blockIdx.y, seq = blockIdx.z;
  const int left = kv_lens[seq] - bi * tpb * 16;  // tokens of this sequence from this block on
  if (left <= 0) return;
  const int blk = block_table[(int64_t)seq * table_stride + bi];
  if (blk < 0) return;
  const int live = min(tpb, (left + 15) >> 4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, n = lane & 15;
  for (int tile = wave; tile < live; tile += 4) {
    const int64_t ti = ((int64_t)blk * n_kv_heads + h) * tpb + tile;
    const uint8_t* sk = k8 + ti * KV8_TILE;
    const uint8_t* sv = v8 + ti * KV8_TILE;
    u32x4 rk[2], rv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rk[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sk + i * 1024 + lane * 16));
      rv[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sv + i * 1024 + lane * 16));
    }
    const float sc_k = *reinterpret_cast<const float*>(sk + KV8_DATA + 4 * n);           // K: the lane's token is n
    const f32x4 sc_v = *reinterpret_cast<const f32x4*>(sv + KV8_DATA + 16 * g);          // V: tokens 4 g .. 4 g + 3
    uint16_t* dk = ks + ti * MI_KV_TILE_ELEMS + lane * 8;
    uint16_t* dv = vs + ti * MI_KV_TILE_ELEMS + lane * 8;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        u32x4 ok, ov;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          const uint32_t qk = rk[i][2 * hh + w], qv = rv[i][2 * hh + w];
          const auto k0 = __builtin_amdgcn_cvt_pk_f32_fp8(qk, false), k1 = __builtin_amdgcn_cvt_pk_f32_fp8(qk, true);
          const auto v0 = __builtin_amdgcn_cvt_pk_f32_fp8(qv, false), v1 = __builtin_amdgcn_cvt_pk_f32_fp8(qv, true);
          ok[2 * w] = pack_bf(k0[0] * sc_k, k0[1] * sc_k);
          ok[2 * w + 1] = pack_bf(k1[0] * sc_k, k1[1] * sc_k);
          ov[2 * w] = pack_bf(v0[0] * sc_v[0], v0[1] * sc_v[1]);
          ov[2 * w + 1] = pack_bf(v1[0] * sc_v[2], v1[1] * sc_v[3]);
        }
        *reinterpret_cast<u32x4*>(dk + (2 * i + hh) * 512) = ok;
        *reinterpret_cast<u32x4*>(dv + (2 * i + hh) * 512) = ov;
      }
  }
}

// ---------------------------------------------------------------------------
// decode attention: grid (splits, n_kv_heads, batch), 8 waves
// ---------------------------------------------------------------------------
struct Chunk8 {  // two tiles as loaded: [tile][load]
  u32x4 k[2][2];
  f32x4 ks[2];
  u32x4 v[2][2];
  f32x4 vs[2];
};

// request order K, K scales, V, V scales: the scores can start while V is still in flight
__device__ __forceinline__ void load_chunk8(const uint8_t* __restrict__ kc_h, const uint8_t* __restrict__ vc_h, int64_t o0,
                                            int64_t o1, int lane, Chunk8& c) {
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const uint8_t* p = kc_h + (tl ? o1 : o0);
#pragma unroll
    for (int i = 0; i < 2; ++i) c.k[tl][i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + i * 1024 + lane * 16));
    c.ks[tl] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + KV8_DATA + (lane >> 4) * 16));
  }
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const uint8_t* p = vc_h + (tl ? o1 : o0);
#pragma unroll
    for (int i = 0; i < 2; ++i) c.v[tl][i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + i * 1024 + lane * 16));
    c.vs[tl] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + KV8_DATA + (lane >> 4) * 16));
  }
}

// scores, online softmax and O^T += V^T . P for one chunk of two tiles starting at token tok0; tokens >= limit are
// masked (wave-uniform limit).  p[0..3] / p[4..7]: tokens 4 g + r of tile 0 / tile 1, column n.
__device__ __forceinline__ void attend_chunk8(const Chunk8& c, const bf16x8 (&Q)[4], int tok0, int limit, float scale_log2e,
                                              int g, float& m, float& l, f32x4 (&acc)[8]) {
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int i = kk >> 1, d = (kk & 1) * 2;
    s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dq8(c.k[0][i][d], c.k[0][i][d + 1]), Q[kk], s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dq8(c.k[1][i][d], c.k[1][i][d + 1]), Q[kk], s1, 0, 0, 0);
  }
  float p[8], vsc[8];
  if (tok0 + 32 <= limit) {  // wave-uniform: the whole chunk is visible
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = s0[r] * (c.ks[0][r] * scale_log2e);  // (a power of two times the scale: the same bits as (s * ks) * scale)
      p[4 + r] = s1[r] * (c.ks[1][r] * scale_log2e);
      vsc[r] = c.vs[0][r];
      vsc[4 + r] = c.vs[1][r];
    }
  } else {  // the scales of unwritten slots are never trusted
    const int t0 = tok0 + 4 * g;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool a = t0 + r < limit, b = t0 + 16 + r < limit;
      p[r] = a ? s0[r] * (c.ks[0][r] * scale_log2e) : -INFINITY;
      p[4 + r] = b ? s1[r] * (c.ks[1][r] * scale_log2e) : -INFINITY;
      vsc[r] = a ? c.vs[0][r] : 0.f;
      vsc[4 + r] = b ? c.vs[1][r] : 0.f;
    }
  }
  float mc = fmaxf(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])), fmaxf(fmaxf(p[4], p[5]), fmaxf(p[6], p[7])));
  mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
  mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
  const float mn = fmaxf(m, mc);
  const bool dead = mn == -INFINITY;  // nothing visible for this column yet
  const float ms = dead ? 0.0f : mn;
  float ps = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    p[i] = __builtin_amdgcn_exp2f(p[i] - ms);
    ps += p[i];
  }
  if (__any(mn != m)) {  // some column's running maximum moved: rescale
    const float alpha = dead ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= alpha;
    m = mn;
  }
  l += ps;  // the sum is over the probabilities; V's scale belongs to the numerator only
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] *= vsc[i];
  u32x4 ph, pl;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ph[i] = pack_bf(p[2 * i], p[2 * i + 1]);
    pl[i] = pack_bf(p[2 * i] - lo_bf(ph[i]), p[2 * i + 1] - hi_bf(ph[i]));
  }
  const bf16x8 Ph = as_frag(ph), Pl = as_frag(pl);
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // dims 16 j ..: dword j % 4 of load j / 4, tile 0 | tile 1
    const u32x2 a0 = dq4(c.v[0][j >> 2][j & 3]), a1 = dq4(c.v[1][j >> 2][j & 3]);
    const bf16x8 a = as_frag(u32x4{a0[0], a0[1], a1[0], a1[1]});
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, Ph, acc[j], 0, 0, 0);
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, Pl, acc[j], 0, 0, 0);
  }
}

// ---- the fused step (FUSE): q/k-norm + RoPE + the quantising store of the step's token inside the attention launch ----
// The new row as the prologue wave publishes it in LDS: K's 128 e4m3 bytes in TILE order (the 16 bytes of lane
// (g, n = token) of fp8 load i at 64 i + 16 g), V's 128 bytes in dim order, then the two scales.
struct NewRow8 {
  __attribute__((aligned(16))) uint8_t k[128];
  __attribute__((aligned(16))) uint8_t v[128];
  float k_scale, v_scale;
};

// Second half of the prologue (the first, step_prologue_issue, ran ahead of the wave's tile loads; all 64 lanes are
// here).  Query heads -> sm_q as bf16.  The k head (pass G / 16, lanes n == G % 16): lane g holds dims 8 g + 32 kk + e of
// the normed, rotated, bf16-rounded row, so the row maximum is a lane-local maximum and two steps over g, and the
// eight bytes of x[kk] are bytes 8 (kk % 2) .. of the lane's 16 bytes of fp8 load kk / 2 - the row is quantised where
// it stands.  The V row (two dims per lane) takes a wave-wide maximum.  Both go to `row` for the wave that attends the
// new token's tile and (k_tile / v_tile non-null: split 0, a real slot) into the cache.
template <int G>
__device__ __forceinline__ void step_prologue_finish8(const StepOperands<G>& o, bool has_norm, float eps, int lane,
                                                      uint8_t* k_tile, uint8_t* v_tile, int tok, uint16_t* sm_q,
                                                      NewRow8& row) {
  const int g = lane >> 4, n = lane & 15;
  u32x4 kq[2] = {};
  float k_scale = 1.f;
#pragma unroll
  for (int ps = 0; ps < StepOperands<G>::PASSES; ++ps) {
    const int hh = n + 16 * ps;
    float x[4][8];
    step_prologue_head<G>(o, ps, has_norm, eps, x);
    if (hh < G) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) *reinterpret_cast<u32x4*>(sm_q + hh * 128 + 8 * g + 32 * kk) = pack16(x[kk]);
    }
    if (ps == G / 16) {  // every lane quantises the head it holds (no divergence around the cross-lane maximum)
      float amax = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[kk][i]));
      amax = xor_max<16>(amax);
      amax = xor_max<32>(amax);
      const int e = kv8_exponent(amax);
      const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
      k_scale = __uint_as_float((uint32_t)(127 + e) << 23);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        kq[kk >> 1][2 * (kk & 1)] = quant4(x[kk][0], x[kk][1], x[kk][2], x[kk][3], inv);
        kq[kk >> 1][2 * (kk & 1) + 1] = quant4(x[kk][4], x[kk][5], x[kk][6], x[kk][7], inv);
      }
    }
  }
  const float v0 = lo_bf(o.v), v1 = hi_bf(o.v);
  const int ev = kv8_exponent(wave_max(fmaxf(fabsf(v0), fabsf(v1))));
  const float inv_v = __uint_as_float((uint32_t)(127 - ev) << 23), v_scale = __uint_as_float((uint32_t)(127 + ev) << 23);
  const uint32_t vq = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v0 * inv_v, v1 * inv_v, 0, false) & 0xffffu;
  const bool k_lane = n == G % 16;
  if (k_lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(row.k + 64 * i + 16 * g) = kq[i];
    if (g == 0) row.k_scale = k_scale;
  }
  *reinterpret_cast<uint16_t*>(row.v + 2 * lane) = (uint16_t)vq;
  if (lane == 0) row.v_scale = v_scale;
  // the cache stores come LAST: loads and stores retire on the same counter, a store in front of a wait would make it
  // wait for the wave's tile loads as well
  if (k_tile != nullptr && k_lane) {  // k8_tile_off(tok, 64 i + 8 g (+ 32)) = i * 1024 + (g * 16 + tok) * 16 (+ 8)
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(k_tile + i * 1024 + (g * 16 + tok) * 16) = kq[i];
    if (g == 0) *reinterpret_cast<float*>(k_tile + KV8_DATA + 4 * tok) = k_scale;
  }
  if (v_tile != nullptr) {
    v_tile[v8_tile_off(tok, 2 * lane)] = (uint8_t)vq;
    v_tile[v8_tile_off(tok, 2 * lane + 1)] = (uint8_t)(vq >> 8);
    if (lane == 0) *reinterpret_cast<float*>(v_tile + KV8_DATA + 4 * tok) = v_scale;
  }
}

// Overwrite token `tok` of tile TL of a loaded chunk with the step's row: the wave that attends the context's last
// tile does not wait for the prologue wave's cache store (a load racing that store sees old or new bytes in exactly
// the places rewritten here).  Of lane (g, n):
//   K load i: the whole quad is token n            -> replaced where n == tok;
//   V load i: dword w = tokens 4 g .. 4 g + 3 of dim 64 i + 16 w + n -> byte tok % 4 where g == tok / 4;
//   scales:   component tok % 4 where g == tok / 4.
// `hit` is wave-uniform; callers patch BOTH tiles of a chunk, each with its own `hit`, through branch-free masks over
// static register indices (paged_attn.hip's patch_new_token says what the alternatives cost).
template <int TL>
__device__ __forceinline__ void patch_new_token8(Chunk8& c, const NewRow8& row, int tok, int g, int n, bool hit) {
  const uint32_t m_k1 = hit && n == tok ? 0xffffffffu : 0u;
  const bool mine = hit && g == (tok >> 2);
  const uint32_t sh = (tok & 3) * 8, m_v1 = mine ? 0xffu << sh : 0u;
  const u32x4 m_k = {m_k1, m_k1, m_k1, m_k1}, m_v = {m_v1, m_v1, m_v1, m_v1};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const u32x4 kn = *reinterpret_cast<const u32x4*>(row.k + 64 * i + 16 * g);
    u32x4 vn;
#pragma unroll
    for (int w = 0; w < 4; ++w) vn[w] = (uint32_t)row.v[64 * i + 16 * w + n] << sh;
    c.k[TL][i] = (c.k[TL][i] & ~m_k) | (kn & m_k);
    c.v[TL][i] = (c.v[TL][i] & ~m_v) | (vn & m_v);
  }
  const float ksn = row.k_scale, vsn = row.v_scale;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool sel = mine && (tok & 3) == r;
    c.ks[TL][r] = sel ? ksn : c.ks[TL][r];
    c.vs[TL][r] = sel ? vsn : c.vs[TL][r];
  }
}

// FUSE = false: q is the [batch][n_q_heads * 128] matrix of prepared query heads and the caches are only read.
// FUSE = true (mi_paged_attn_decode_fp8kv_fused): q is the packed qkv matrix, fs the prologue's operands; the last
// wave of the workgroup (never a long run, see deal()) runs the prologue, split 0 writes the new row into the caches.
template <int G, bool FUSE>
__global__ __launch_bounds__(512) void paged_attn_decode_fp8kv_kernel(
    const uint16_t* __restrict__ q, int64_t q_stride, const uint8_t* kc, const uint8_t* vc,
    const int32_t* __restrict__ block_table, int table_stride, const int32_t* __restrict__ ctx_lens,
    float* __restrict__ part_o, float* __restrict__ part_ml, uint16_t* __restrict__ out, int n_q_heads, int tpb,
    int tpb_shift, float scale_log2e, FusedStep fs) {
  constexpr int WAVES = 8, D = 128;
  __shared__ __attribute__((aligned(16))) float sm_o[WAVES][G][D];
  __shared__ float sm_m[WAVES][16];
  __shared__ float sm_l[WAVES][16];
  __shared__ __attribute__((aligned(16))) uint16_t sm_q[G][D];
  __shared__ NewRow8 sm_new;  // FUSE: the step's K / V row, quantised

  const int split = blockIdx.x, splits = gridDim.x, h = blockIdx.y, b = blockIdx.z, n_kv_heads = gridDim.y;
  const int ctx = max(ctx_lens[b], 0);
  const int n_tiles = (ctx + 15) >> 4;
  // chunks of two tiles dealt to the WAVES * splits waves as evenly as possible, each wave a contiguous run (the
  // bf16 kernel's deal: sizes differ by at most one, the longer runs first)
  const int n_chunks = (n_tiles + 1) >> 1, n_waves = WAVES * splits;
  const int deal_q = n_chunks / n_waves, deal_r = n_chunks % n_waves;
  auto deal = [&](int r) { return r * deal_q + min(r, deal_r); };
  const int wg_c0 = deal(split * WAVES), wg_c1 = deal((split + 1) * WAVES);
  const int64_t row0 = (int64_t)b * n_q_heads + h * G;
  if (wg_c0 >= wg_c1) {  // uniform for the workgroup: nothing to attend in this split
    if (splits == 1) {   // empty context (graph padding row): the output row is zero
      for (int idx = threadIdx.x; idx < G * (D / 2); idx += WAVES * 64)
        *reinterpret_cast<uint32_t*>(out + row0 * D + 2 * idx) = 0u;
    } else {
      for (int hn = threadIdx.x; hn < G; hn += WAVES * 64) {
        part_ml[((row0 + hn) * 16 + split) * 2] = -INFINITY;
        part_ml[((row0 + hn) * 16 + split) * 2 + 1] = 0.f;
      }
    }
    return;
  }

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int32_t* table_row = block_table + (int64_t)b * table_stride;
  const int vw = split * WAVES + wave;
  const int t0 = 2 * deal(vw), t1 = min(n_tiles, 2 * deal(vw + 1));

  // FUSE: the token of this step sits at position ctx - 1, row new_tok of tile new_tile.  The prologue wave's
  // operands (and the slot) are requested here, ahead of its tile loads.
  const int new_tile = (ctx - 1) >> 4, new_tok = (ctx - 1) & 15;
  const bool is_pro = FUSE && wave == WAVES - 1;
  StepOperands<G> pro;
  int32_t blk = 0, off = 0;
  if (is_pro) {
    blk = fs.slots[2 * b];
    off = fs.slots[2 * b + 1];
    step_prologue_issue<G>(pro, q + (int64_t)b * q_stride, n_q_heads, n_kv_heads, h, fs,
                           fs.cos_sin + fs.positions[b] * 128, lane);
  }
  auto finish_prologue = [&]() __attribute__((always_inline)) {
    const bool store = split == 0 && blk >= 0 && off >= 0;  // split 0 always has work (the longer runs come first)
    const int64_t tile_w = kv8_tile_base(blk, h, off, n_kv_heads, tpb);
    step_prologue_finish8<G>(pro, fs.q_w != nullptr, fs.eps, lane, store ? const_cast<uint8_t*>(kc) + tile_w : nullptr,
                             store ? const_cast<uint8_t*>(vc) + tile_w : nullptr, off & 15, &sm_q[0][0], sm_new);
  };

  if (!FUSE && wave == 0) {  // stage the G query heads (contiguous G * 256 bytes of the q row)
    for (int c = lane; c < G * (D / 8); c += 64)
      *reinterpret_cast<u32x4*>(&sm_q[0][0] + 8 * c) =
          *reinterpret_cast<const u32x4*>(q + (int64_t)b * q_stride + (int64_t)h * G * D + 8 * c);
  }

  float m = -INFINITY, l = 0.f;
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t block_bytes = (int64_t)n_kv_heads * tpb * KV8_TILE;
  const uint8_t* const kc_h = kc + (int64_t)h * tpb * KV8_TILE;
  const uint8_t* const vc_h = vc + (int64_t)h * tpb * KV8_TILE;
  // a single-tile chunk loads its tile twice (a cache hit) and masks the duplicate through the limit
  auto second = [&](int t) { return t + 1 < t1 ? t + 1 : t; };
  auto limit_of = [&](int t) { return t + 1 < t1 ? ctx : min(ctx, (t + 1) * 16); };
  auto tile_off = [&](int t) __attribute__((always_inline)) -> int64_t {
    const int bi = tpb_shift >= 0 ? t >> tpb_shift : t / tpb;
    const int in_block = tpb_shift >= 0 ? t & (tpb - 1) : t % tpb;
    return (int64_t)table_row[bi] * block_bytes + (int64_t)in_block * KV8_TILE;
  };
  // Two chunk buffers.  Every path below is straight-line in its loads, so the compiler's vmcnt bookkeeping is exact:
  // an attend waits for its own buffer while the other buffer's 12 loads stay in flight behind it.
  Chunk8 A, B;
  bf16x8 Q[4];
  int ta = t0, tb = t0 + 2;
  auto load_a = [&]() __attribute__((always_inline)) { load_chunk8(kc_h, vc_h, tile_off(ta), tile_off(second(ta)), lane, A); };
  auto load_b = [&]() __attribute__((always_inline)) { load_chunk8(kc_h, vc_h, tile_off(tb), tile_off(second(tb)), lane, B); };
  auto attend_a = [&]() __attribute__((always_inline)) {
    if constexpr (FUSE) {
      if (ta == new_tile || ta + 1 == new_tile) {  // wave-uniform, true once per (sequence, kv head)
        patch_new_token8<0>(A, sm_new, new_tok, g, n, ta == new_tile);
        patch_new_token8<1>(A, sm_new, new_tok, g, n, ta + 1 == new_tile);
      }
    }
    attend_chunk8(A, Q, ta * 16, limit_of(ta), scale_log2e, g, m, l, acc);
  };
  auto attend_b = [&]() __attribute__((always_inline)) {
    if constexpr (FUSE) {
      if (tb == new_tile || tb + 1 == new_tile) {
        patch_new_token8<0>(B, sm_new, new_tok, g, n, tb == new_tile);
        patch_new_token8<1>(B, sm_new, new_tok, g, n, tb + 1 == new_tile);
      }
    }
    attend_chunk8(B, Q, tb * 16, limit_of(tb), scale_log2e, g, m, l, acc);
  };
  auto load_q = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      u32x4 v = *reinterpret_cast<const u32x4*>(&sm_q[n < G ? n : 0][8 * g + 32 * kk]);
      if (n >= G) v = u32x4{0, 0, 0, 0};
      Q[kk] = as_frag(v);
    }
  };
  if (tb < t1) {  // at least two chunks
    load_a();
    if (is_pro) finish_prologue();  // under the latency of buffer A
    load_b();
    __syncthreads();  // sm_q (FUSE: and the new row) complete; this wave's tile loads are in flight behind the barrier
    load_q();
    while (tb + 4 < t1) {  // both buffers have a successor
      attend_a();
      ta += 4;
      load_a();
      attend_b();
      tb += 4;
      load_b();
    }
    attend_a();
    if (ta + 4 < t1) {  // one more chunk behind B
      ta += 4;
      load_a();
      attend_b();
      attend_a();
    } else {
      attend_b();
    }
  } else if (ta < t1) {  // a single chunk
    load_a();
    if (is_pro) finish_prologue();
    __syncthreads();
    load_q();
    attend_a();
  } else {
    if (is_pro) finish_prologue();
    __syncthreads();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);

  if (n < G) {
#pragma unroll
    for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(&sm_o[wave][n][j * 16 + 4 * g]) = acc[j];
    if (g == 0) {
      sm_m[wave][n] = m;
      sm_l[wave][n] = l;
    }
  }
  __syncthreads();
  // merge the waves (at least one of them had a chunk, so M is finite; empty ones weigh exp2(-inf) = 0)
  for (int idx = threadIdx.x; idx < G * D; idx += WAVES * 64) {
    const int hn = idx / D, d = idx % D;
    float M = sm_m[0][hn];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) M = fmaxf(M, sm_m[w][hn]);
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const float e = exp2f(sm_m[w][hn] - M);
      o += e * sm_o[w][hn][d];
      L += e * sm_l[w][hn];
    }
    if (splits == 1) {
      out[(row0 + hn) * D + d] = f2bf(o / L);
    } else {
      const int64_t slot = (row0 + hn) * 16 + split;
      part_o[slot * D + d] = o;
      if (d == 0) {
        part_ml[slot * 2] = M;
        part_ml[slot * 2 + 1] = L;
      }
    }
  }
}

// merge the splits (small batches only): one wave per (sequence, q head) row, lane = 2 dims; the partials have the
// layout of mi_paged_attn_decode's workspace
__global__ __launch_bounds__(256) void paged_attn_merge_fp8kv_kernel(const float* __restrict__ part_o,
                                                                     const float* __restrict__ part_ml,
                                                                     uint16_t* __restrict__ out, int n_rows, int splits) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  float ms = -INFINITY, ls = 0.f;
  if (lane < splits) {
    const float2 ml = *reinterpret_cast<const float2*>(part_ml + (row * 16 + lane) * 2);
    ms = ml.x;
    ls = ml.y;
  }
  const float M = wave_max(ms);
  const float e = (lane < splits && ms != -INFINITY) ? exp2f(ms - M) : 0.f;
  const float den = wave_sum(e * ls);
  float2 acc = {0.f, 0.f};
  for (int s = 0; s < splits; ++s) {
    const float es = __shfl(e, s, 64);
    if (es != 0.f) {  // (wave-uniform; empty splits never wrote their partial rows)
      const float2 o = *reinterpret_cast<const float2*>(part_o + (row * 16 + s) * 128 + 2 * lane);
      acc.x += es * o.x;
      acc.y += es * o.y;
    }
  }
  const float inv = den > 0.f ? 1.0f / den : 0.f;
  *reinterpret_cast<uint32_t*>(out + row * 128 + 2 * lane) = pack_bf(acc.x * inv, acc.y * inv);
}

// splits per (sequence, kv head): aim at ~16 waves per CU over the whole launch (the bf16 kernel's rule)
static int decode_splits8(int batch, int n_kv_heads) {
  const int base = batch * n_kv_heads * 16;
  const int ns = 4096 / (base > 0 ? base : 1);
  return ns < 1 ? 1 : (ns > 16 ? 16 : ns);
}

}  // namespace mi

using namespace mi;

extern "C" int mi_kv_store_fp8(const mi_bf16* k, const mi_bf16* v, int64_t k_row_stride, int64_t v_row_stride,
                               uint8_t* k_cache, uint8_t* v_cache, const int32_t* slots, int slot_is_2d, int n_tokens,
                               int n_kv_heads, int head_dim, int block_size, mi_stream stream) {
  if (!k || !v || !k_cache || !v_cache || !slots || n_tokens < 0) return MI_EINVAL;
  int rc = check_kv8(n_kv_heads, head_dim, block_size);
  if (rc != MI_OK) return rc;
  if (k_row_stride % 8 || v_row_stride % 8) return MI_EUNSUPPORTED;
  if (!aligned16(k) || !aligned16(v) || !aligned16(k_cache) || !aligned16(v_cache)) return MI_EINVAL;
  if (n_tokens == 0) return MI_OK;
  const int64_t lanes = (int64_t)n_tokens * n_kv_heads * 2 * 8;
  hipLaunchKernelGGL(kv_store_fp8_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, S(stream), k, v, k_row_stride,
                     v_row_stride, k_cache, v_cache, slots, slot_is_2d, n_tokens, n_kv_heads, block_size);
  return check_launch();
}

extern "C" int mi_kv_cache_gather_fp8(const uint8_t* cache, int is_v, const int32_t* slot_flat, int n, uint8_t* out_q,
                                      float* out_scale, int n_kv_heads, int head_dim, int block_size, mi_stream stream) {
  if (!cache || !slot_flat || !out_q || !out_scale || n < 0) return MI_EINVAL;
  int rc = check_kv8(n_kv_heads, head_dim, block_size);
  if (rc != MI_OK || n == 0) return rc;
  const int64_t total = (int64_t)n * n_kv_heads * 128;
  hipLaunchKernelGGL(kv_gather_fp8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(stream), cache, is_v,
                     slot_flat, n, out_q, out_scale, n_kv_heads, block_size);
  return check_launch();
}

extern "C" int mi_kv_fp8_expand(const uint8_t* k_cache, const uint8_t* v_cache, mi_bf16* k_scratch, mi_bf16* v_scratch,
                                const int32_t* block_table, int table_stride, const int32_t* kv_lens, int n_seqs,
                                int n_kv_heads, int head_dim, int block_size, mi_stream stream) {
  if (!k_cache || !v_cache || !k_scratch || !v_scratch || !block_table || !kv_lens || n_seqs < 0 || table_stride <= 0)
    return MI_EINVAL;
  int rc = check_kv8(n_kv_heads, head_dim, block_size);
  if (rc != MI_OK) return rc;
  if (!aligned16(k_cache) || !aligned16(v_cache) || !aligned16(k_scratch) || !aligned16(v_scratch)) return MI_EINVAL;
  if (n_seqs == 0) return MI_OK;
  if (n_kv_heads > 65535 || n_seqs > 65535) return MI_EUNSUPPORTED;
  hipLaunchKernelGGL(kv_fp8_expand_kernel, dim3(table_stride, n_kv_heads, n_seqs), dim3(256), 0, S(stream), k_cache, v_cache,
                     k_scratch, v_scratch, block_table, table_stride, kv_lens, n_kv_heads, block_size / 16);
  return check_launch();
}

// both decode entry points: fused == nullptr attends prepared query heads, otherwise q is the packed qkv matrix
static int decode8_impl(const mi_bf16* q, int64_t q_row_stride, const uint8_t* k_cache, const uint8_t* v_cache,
                        const int32_t* block_table, int table_stride, const int32_t* context_lens, mi_bf16* out,
                        void* workspace, size_t ws_bytes, int batch, int n_q_heads, int n_kv_heads, int head_dim,
                        int block_size, float scale, mi_stream stream, const FusedStep* fused) {
  if (!q || !k_cache || !v_cache || !block_table || !context_lens || !out || !workspace) return MI_EINVAL;
  if (n_q_heads <= 0 || batch < 0 || table_stride <= 0) return MI_EINVAL;
  int rc = check_kv8(n_kv_heads, head_dim, block_size);
  if (rc != MI_OK) return rc;
  if (q_row_stride % 8 || n_q_heads % n_kv_heads) return MI_EUNSUPPORTED;
  const int G = n_q_heads / n_kv_heads;
  if (G != 1 && G != 2 && G != 4 && G != 8 && G != 16) return MI_EUNSUPPORTED;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out) || !aligned16(workspace)) return MI_EINVAL;
  if (batch == 0) return MI_OK;
  if (batch > 65535 || n_kv_heads > 65535) return MI_EUNSUPPORTED;
  if (ws_bytes < mi_paged_attn_decode_workspace(batch, n_q_heads)) return MI_EWORKSPACE;
  const int nsplit = decode_splits8(batch, n_kv_heads);
  float* part_o = static_cast<float*>(workspace);
  float* part_ml = part_o + (size_t)batch * n_q_heads * 16 * 128;
  const float sl2 = scale * 1.4426950408889634f;
  const int tpb = block_size / 16;
  int tpb_shift = -1;  // log2 of the tiles per block, or -1 (division) for block sizes like 48
  for (int sft = 0; sft < 12; ++sft)
    if ((1 << sft) == tpb) tpb_shift = sft;
  const dim3 grid(nsplit, n_kv_heads, batch);
  hipStream_t st = S(stream);
  const FusedStep fs = fused ? *fused : FusedStep{};
#define LAUNCH_DEC8_AS(GG, FF)                                                                                          \
  hipLaunchKernelGGL((paged_attn_decode_fp8kv_kernel<GG, FF>), grid, dim3(512), 0, st, q, q_row_stride, k_cache, v_cache, \
                     block_table, table_stride, context_lens, part_o, part_ml, out, n_q_heads, tpb, tpb_shift, sl2, fs)
#define LAUNCH_DEC8(GG)                   \
  if (fused) LAUNCH_DEC8_AS(GG, true);    \
  else LAUNCH_DEC8_AS(GG, false)
  switch (G) {
    case 1: LAUNCH_DEC8(1); break;
    case 2: LAUNCH_DEC8(2); break;
    case 4: LAUNCH_DEC8(4); break;
    case 8: LAUNCH_DEC8(8); break;
    default: LAUNCH_DEC8(16); break;
  }
#undef LAUNCH_DEC8
#undef LAUNCH_DEC8_AS
  rc = check_launch();
  if (rc != MI_OK || nsplit == 1) return rc;
  const int rows = batch * n_q_heads;
  hipLaunchKernelGGL(paged_attn_merge_fp8kv_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, part_o, part_ml, out, rows, nsplit);
  return check_launch();
}

extern "C" int mi_paged_attn_decode_fp8kv(const mi_bf16* q, int64_t q_row_stride, const uint8_t* k_cache,
                                          const uint8_t* v_cache, const int32_t* block_table, int table_stride,
                                          const int32_t* context_lens, mi_bf16* out, void* workspace, size_t ws_bytes,
                                          int batch, int n_q_heads, int n_kv_heads, int head_dim, int block_size,
                                          float scale, mi_stream stream) {
  return decode8_impl(q, q_row_stride, k_cache, v_cache, block_table, table_stride, context_lens, out, workspace, ws_bytes,
                      batch, n_q_heads, n_kv_heads, head_dim, block_size, scale, stream, nullptr);
}

// qwen3.py:79-90 + attention.py:32-35,63-93 over the fp8 cache: the launches mi_rmsnorm (q), mi_rmsnorm (k), mi_rope,
// mi_kv_store_fp8 and mi_paged_attn_decode_fp8kv in one
extern "C" int mi_paged_attn_decode_fp8kv_fused(const mi_bf16* qkv, int64_t qkv_row_stride, const mi_bf16* q_w,
                                                const mi_bf16* k_w, float eps, const int64_t* positions,
                                                const float* cos_sin, const int32_t* slot_2d, uint8_t* k_cache,
                                                uint8_t* v_cache, const int32_t* block_table, int table_stride,
                                                const int32_t* context_lens, mi_bf16* out, void* workspace,
                                                size_t ws_bytes, int batch, int n_q_heads, int n_kv_heads, int head_dim,
                                                int block_size, float scale, mi_stream stream) {
  if (!positions || !cos_sin || !slot_2d) return MI_EINVAL;
  if ((q_w == nullptr) != (k_w == nullptr)) return MI_EINVAL;
  if (!aligned16(cos_sin) || (q_w && (!aligned16(q_w) || !aligned16(k_w)))) return MI_EINVAL;
  const FusedStep fs{q_w, k_w, positions, cos_sin, slot_2d, eps};
  return decode8_impl(qkv, qkv_row_stride, k_cache, v_cache, block_table, table_stride, context_lens, out, workspace,
                      ws_bytes, batch, n_q_heads, n_kv_heads, head_dim, block_size, scale, stream, &fs);
}
