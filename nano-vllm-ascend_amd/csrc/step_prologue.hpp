// The step prologue that the fused decode attention launches share (paged_attn.hip over the bf16 cache,
// paged_attn_fp8kv.hip over the fp8 one): operands, their loads, and the q/k RMSNorm + RoPE arithmetic on the
// MFMA-operand distribution of a head.  What differs between the two - how the new K / V row reaches LDS and the
// cache - stays with each kernel.
#pragma once
#include "mi_common.hpp"
#include "kv_store.hpp"

namespace mi {

// Operands of the fused step prologue (FUSE): the packed qkv row of QKVParallelLinear is consumed
// directly - q_norm / k_norm / RoPE (qwen3.py:83-88) and the scatter of the new token's K / V row
// (attention.py:32-35) happen inside the attention launch (bit-identical to mi_qknorm_rope_store,
// same helpers).
struct FusedStep {
  const uint16_t* q_w;        // [128] or nullptr (attention_bias models have no q/k norm)
  const uint16_t* k_w;
  const int64_t* positions;   // [batch]
  const float* cos_sin;       // [max_pos][128] fp32
  const int32_t* slots;       // [batch][2] = {block id, offset}
  float eps;
};

// Step prologue of the fused launch, run by ONE wavefront per workgroup.  Lane (g, n) takes head
// hh = n (+16 for a second pass when G = 16) of {the G query heads of kv head h, then its k head}, dims
// 8g + 32kk + e.  The operand loads are ISSUED before the wave's K/V tile loads (vmcnt retires in
// order: they can then be waited for without waiting for the tiles) and CONSUMED behind them, so the
// prologue's arithmetic runs under the tile loads' latency.
template <int G>
struct StepOperands {
  static constexpr int PASSES = (G + 1 + 15) / 16;
  u32x4 x[PASSES][4], w[PASSES][4];
  float4 cs[8];  // cos(8g..), cos(8g+4..), sin(..), sin(..) for the pair (kk0, kk2), then for (kk1, kk3)
  uint32_t v;    // two dims of the V row
};

template <int G>
__device__ __forceinline__ void step_prologue_issue(StepOperands<G>& o, const uint16_t* row, int n_q_heads, int n_kv,
                                                    int h, const FusedStep& fs, const float* cs, int lane) {
  const int g = lane >> 4, n = lane & 15;
#pragma unroll
  for (int ps = 0; ps < StepOperands<G>::PASSES; ++ps) {
    const int hh = min(n + 16 * ps, G);  // lanes beyond the last head shadow the k head (results unused)
    const bool is_k = hh == G;
    const uint16_t* src = row + (int64_t)(is_k ? n_q_heads + h : h * G + hh) * 128 + 8 * g;
    const uint16_t* w = is_k ? fs.k_w : fs.q_w;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      o.x[ps][kk] = *reinterpret_cast<const u32x4*>(src + 32 * kk);
      if (w != nullptr) o.w[ps][kk] = *reinterpret_cast<const u32x4*>(w + 8 * g + 32 * kk);
    }
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float* cp = cs + 32 * p + 8 * g;
    o.cs[4 * p + 0] = *reinterpret_cast<const float4*>(cp);
    o.cs[4 * p + 1] = *reinterpret_cast<const float4*>(cp + 4);
    o.cs[4 * p + 2] = *reinterpret_cast<const float4*>(cp + 64);
    o.cs[4 * p + 3] = *reinterpret_cast<const float4*>(cp + 68);
  }
  o.v = *reinterpret_cast<const uint32_t*>(row + (int64_t)(n_q_heads + n_kv + h) * 128 + 2 * lane);
}

// The head of pass ps, normed and rotated: x[kk][e] = dim 8g + 32kk + e, every value a bf16.  q/k RMSNorm + RoPE
// with the rounding points (and the summation order) of head_rmsnorm / head_rope in kv_store.hpp.
template <int G>
__device__ __forceinline__ void step_prologue_head(const StepOperands<G>& o, int ps, bool has_norm, float eps,
                                                   float (&x)[4][8]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[kk][2 * j] = lo_bf(o.x[ps][kk][j]);
      x[kk][2 * j + 1] = hi_bf(o.x[ps][kk][j]);
    }
  if (has_norm) {  // head_rmsnorm_frag with the weights already in registers
    float lo = 0.f, hi = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) lo += x[0][i] * x[0][i];
#pragma unroll
    for (int i = 0; i < 8; ++i) lo += x[2][i] * x[2][i];
#pragma unroll
    for (int i = 0; i < 8; ++i) hi += x[1][i] * x[1][i];
#pragma unroll
    for (int i = 0; i < 8; ++i) hi += x[3][i] * x[3][i];
    lo += __shfl_xor(lo, 16, 64);
    lo += __shfl_xor(lo, 32, 64);
    hi += __shfl_xor(hi, 16, 64);
    hi += __shfl_xor(hi, 32, 64);
    const float rs = 1.0f / sqrtf((lo + hi) / 128.0f + eps);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[kk][2 * j] = rbf(rbf(x[kk][2 * j] * rs) * lo_bf(o.w[ps][kk][j]));
        x[kk][2 * j + 1] = rbf(rbf(x[kk][2 * j + 1] * rs) * hi_bf(o.w[ps][kk][j]));
      }
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float c[8] = {o.cs[4 * p].x, o.cs[4 * p].y, o.cs[4 * p].z, o.cs[4 * p].w,
                        o.cs[4 * p + 1].x, o.cs[4 * p + 1].y, o.cs[4 * p + 1].z, o.cs[4 * p + 1].w};
    const float sn[8] = {o.cs[4 * p + 2].x, o.cs[4 * p + 2].y, o.cs[4 * p + 2].z, o.cs[4 * p + 2].w,
                         o.cs[4 * p + 3].x, o.cs[4 * p + 3].y, o.cs[4 * p + 3].z, o.cs[4 * p + 3].w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x1 = x[p][i], x2 = x[p + 2][i];
      x[p][i] = rbf(x1 * c[i] - x2 * sn[i]);
      x[p + 2][i] = rbf(x2 * c[i] + x1 * sn[i]);
    }
  }
}

}  // namespace mi
