// Weight-streaming GEMM over int4 (group-128) weights: y[M][N] = x[M][K] @ (dequantised w[N][K])^T.
//
// Format (include/mi355_nanovllm.h): nibble q in 0..15, one bf16 scale s per (row, group of 128 k) whose significand
// has four bits; the weight is (q - 8) * s - a four-bit integer times a four-bit significand: EXACT in bf16.
//   packed nibbles [N/16][K/128][64 lanes][16 B]: lane (g, r) holds the A-fragment values of row 16 tn + r for the four
//     32-deep k-steps of group tk; dword s = the eight nibbles of k = 128 tk + 32 s + 8 g + e, element e at bits 4 e.
//     One wave-load is one contiguous 1 KiB, as in the bf16 and fp8 layouts, and feeds FOUR k-steps.
//   packed scales  [N/16][K/128][16] bf16 in row order: 32 bytes per (row tile, group); the four rows of a lane's C
//     fragment are 8 contiguous bytes, the row of its A fragment one element.
//
// Which side carries the scale.  gfx950 has no packed bf16 arithmetic (v_pk_add_bf16 arrives with a later ISA), so the
// OR-a-magic-exponent form (0x4300 | q = 128 + q) cannot finish its subtraction in bf16: unpacked to fp32, subtracted
// and packed again it costs 27 VALU per dword.  The cheapest exact expansion found goes through fp32 anyway:
//     two masks (d & 0x0f0f0f0f, d & 0xf0f0f0f0) -> eight v_cvt_f32_ubyteN -> four v_pk_fma_f32 -> four v_cvt_pk_bf16_f32
// and in that form the fp32 operation that subtracts the 8 can multiply by the scale for free:
//     a = q * s - 8 s          (even elements)        a = (16 q) * (s / 16) - 8 s          (odd elements, unshifted)
// Both are exact ((q - 8) s has at most eight significant bits, s / 16 is a power-of-two step), so the A fragment holds
// the dequantised bf16 weight itself.  That is the form kept here: it needs no group accumulator (RT * MT * 4 more VGPRs,
// their zeroing and 4 * RT * MT folding FMAs per group), reads ONE scale per lane and group instead of four, and the
// MFMAs see exactly the operands of a bf16 GEMM over the dequantised weight.  The group-accumulator
// form would save nothing in the expansion: its subtraction is the same v_pk instruction as this multiply-add.
// Counted in the disassembly: 18 VALU per dword, 72 per 16-byte load (+ 3 per group for s, s / 16, -8 s).
//
// Loop: the bf16 kernel's double-buffered form (gemm_skinny_kernel.hpp, PIPE) on blocks of one group - two named
// register sets {weights, scale, x lines}, the loads of group i + 1 issued before group i is expanded, the tail
// peeled, no conditional load.  x goes through the per-wave LDS slab as whole cache lines (issue_x_lines /
// x_lines_to_frags).  Everything after the K-slices is the bf16 kernel's: sums through LDS in wave order, the SiLU
// epilogue with the reference's rounding points, fp32 partials for split-K, row chunks of 64 on blockIdx.z.
#pragma once
#include "gemm_skinny_kernel.hpp"

namespace mi {

typedef __attribute__((ext_vector_type(2))) float f32x2;

// float(byte J of v).  Written as inline assembly: from `(float)((v >> 8 J) & 0xff)` the compiler, knowing the masked
// bytes' upper bits, extracts every byte with an SDWA `and` first and converts with v_cvt_f32_ubyte0 only (+ 4 VALU
// per dword).
template <int J>
__device__ __forceinline__ float ubyte_f32(uint32_t v) {
  float f;
  if constexpr (J == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(v));
  if constexpr (J == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(v));
  if constexpr (J == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(v));
  if constexpr (J == 3) asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(v));
  return f;
}

// the A fragment (eight bf16) of one k-step from its dword of nibbles; mul = {s, s / 16}, add = {-8 s, -8 s}
__device__ __forceinline__ u32x4 int4_expand(uint32_t d, f32x2 mul, f32x2 add) {
  const uint32_t lo = d & 0x0f0f0f0fu, hi = d & 0xf0f0f0f0u;  // even elements as bytes; odd elements as bytes, times 16
  const f32x2 q[4] = {{ubyte_f32<0>(lo), ubyte_f32<0>(hi)}, {ubyte_f32<1>(lo), ubyte_f32<1>(hi)},
                      {ubyte_f32<2>(lo), ubyte_f32<2>(hi)}, {ubyte_f32<3>(lo), ubyte_f32<3>(hi)}};
  u32x4 a;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 v = __builtin_elementwise_fma(q[j], mul, add);  // v_pk_fma_f32
    a[j] = pack_bf(v[0], v[1]);                                 // v_cvt_pk_bf16_f32 (exact)
  }
  return a;
}

// Kernel arguments: x .. kslice are the ten dwords in front of the first vector load and y / part complete the
// fourteen-dword prefix that arrives in SGPRs (kernarg preload, see the Makefile).
// ONE: the K-slice of a wave is a single group (every projection of a hidden-1024 model but down_proj) - no second
// register set, so that 16 waves fit where the double-buffered loop would not.
template <int MT, int RT, int WAVES, int EPI, bool ONE>
__global__ __launch_bounds__(WAVES * 64) void gemm_int4w_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const uint16_t* __restrict__ sc, int M_all, int N,
    int K, int kslice, uint16_t* __restrict__ y, float* __restrict__ part) {
  const int m0 = (int)blockIdx.z * kSkinnyRows;  // more than 64 activation rows: chunks of 64, as gemm_skinny_kernel
  const int M = min(M_all - m0, kSkinnyRows);
  x += (int64_t)m0 * K;
  if (y) y += (int64_t)m0 * (EPI == EPI_SILU ? N >> 1 : N);
  // [WAVES][RT*MT][256] fp32 K-slice sums; before that, each wave's slot doubles as its x slab
  extern __shared__ __attribute__((aligned(16))) float red[];
  constexpr int SLOT = RT * MT * 1024 > x_slab_bytes(MT) ? RT * MT * 1024 : x_slab_bytes(MT);  // bytes per wave
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15;
  uint16_t* slab = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(red) + wave * SLOT);
  // kslice = K / (gridDim.y * WAVES), a multiple of 128, computed and checked on the host
  const int kbeg = (blockIdx.y * WAVES + wave) * kslice;
  const int kgroups = K >> 7;

  int tile[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
    tile[t] = EPI == EPI_SILU ? (int)blockIdx.x + t * (N >> 5) : (int)blockIdx.x * RT + t;

  f32x4 acc[RT][MT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint8_t* wp[RT];   // this lane's 16 bytes of the wave's first group
  const uint16_t* sp[RT];  // the scale of its A-fragment row
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t grp = (int64_t)tile[t] * kgroups + (kbeg >> 7);
    wp[t] = w + grp * 1024 + lane * 16;
    sp[t] = sc + grp * 16 + r;
  }

  u32x4 aA[RT], stA[2][MT * 2];
  uint16_t sA[RT];
  auto issue = [&](u32x4(&a)[RT], uint16_t(&s)[RT], u32x4(&st)[2][MT * 2], int grp) {
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      a[t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[t] + grp * 1024));
      s[t] = sp[t][grp * 16];
    }
    issue_x_lines<MT, 4>(x, M, K, kbeg + grp * 128, lane, st);
    // nothing of the group being consumed may be scheduled above these loads (see the bf16 kernel's PIPE loop)
    __builtin_amdgcn_sched_barrier(0);
  };
  auto consume = [&](const u32x4(&a)[RT], const uint16_t(&s)[RT], const u32x4(&st)[2][MT * 2]) {
    u32x4 bfrag[MT][4];
    x_lines_to_frags<MT, 4>(st, slab, lane, bfrag);
    f32x2 mul[RT], add[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const float sf = bf2f(s[t]);
      mul[t] = f32x2{sf, sf * 0.0625f};
      add[t] = f32x2{-8.0f * sf, -8.0f * sf};
    }
#pragma unroll
    for (int st4 = 0; st4 < 4; ++st4)
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const u32x4 af = int4_expand(a[t][st4], mul[t], add[t]);
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af), as_frag(bfrag[m][st4]), acc[t][m], 0, 0, 0);
      }
  };
  issue(aA, sA, stA, 0);
  if constexpr (ONE) {
    consume(aA, sA, stA);
  } else {
    u32x4 aB[RT], stB[2][MT * 2];
    uint16_t sB[RT];
    const int n = kslice >> 7;
    int it = 0;
    for (; it + 2 < n; it += 2) {
      issue(aB, sB, stB, it + 1);
      consume(aA, sA, stA);
      issue(aA, sA, stA, it + 2);
      consume(aB, sB, stB);
    }
    if (it + 1 < n) {
      issue(aB, sB, stB, it + 1);
      consume(aA, sA, stA);
      consume(aB, sB, stB);
    } else {
      consume(aA, sA, stA);
    }
  }

  // C fragment: lane (g, c) holds y[m-tile col c][16 tile + 4 g + i], i = 0..3
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m)
      *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(red) + wave * SLOT + ((t * MT + m) * 64 + lane) * 16) = acc[t][m];
  __syncthreads();
  // each (row tile, m-tile, lane) result is finished by one thread, summing K-slices in wave order
  constexpr int ITEMS = (EPI == EPI_SILU ? 1 : RT) * MT * 64;
  for (int item = threadIdx.x; item < ITEMS; item += WAVES * 64) {
    const int l = item & 63, m = (item >> 6) % MT, t = (item >> 6) / MT;
    auto total = [&](int tt) {
      f32x4 s = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(red) + ((tt * MT + m) * 64 + l) * 16);
#pragma unroll
      for (int wv = 1; wv < WAVES; ++wv)
        s += *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(red) + wv * SLOT + ((tt * MT + m) * 64 + l) * 16);
      return s;
    };
    const int row = 16 * m + (l & 15);
    if (row >= M) continue;
    if (EPI == EPI_SILU) {
      const f32x4 gt = total(0), up = total(1);
      const int col = (int)blockIdx.x * 16 + 4 * (l >> 4);
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gb = rbf(gt[i]);  // the gate_up GEMM output, rounded to bf16 as the unfused path
        const float sb = rbf(gb / (1.0f + expf(-gb)));
        o[i] = sb * rbf(up[i]);
      }
      *reinterpret_cast<u32x2*>(y + (int64_t)row * (N >> 1) + col) = u32x2{pack_bf(o[0], o[1]), pack_bf(o[2], o[3])};
    } else {
      const f32x4 s = total(t);
      const int col = tile[0] * 16 + t * 16 + 4 * (l >> 4);
      if (EPI == EPI_PARTIAL)
        *reinterpret_cast<f32x4*>(part + ((int64_t)blockIdx.y * M_all + m0 + row) * N + col) = s;
      else
        *reinterpret_cast<u32x2*>(y + (int64_t)row * N + col) = u32x2{pack_bf(s[0], s[1]), pack_bf(s[2], s[3])};
    }
  }
}

// Row-major (q [N][K] one nibble per byte, scale [N][K/128] bf16) -> the two packed layouts.  One thread per 16
// packed bytes; the lanes of the first k-group also place the sixteen scales of their (row tile, group).
static __global__ __launch_bounds__(256) void pack_weight_int4_kernel(const uint8_t* __restrict__ q,
                                                                      const uint16_t* __restrict__ scale,
                                                                      uint8_t* __restrict__ dst,
                                                                      uint16_t* __restrict__ dst_scale, int N, int K) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)N * K / 32) return;
  const int lane = idx & 63, g = lane >> 4, r = lane & 15;
  const int64_t frag = idx >> 6;
  const int kgroups = K >> 7;
  const int tk = frag % kgroups;
  const int64_t tn = frag / kgroups;
  const uint8_t* row = q + (tn * 16 + r) * K + tk * 128 + g * 8;
  u32x4 v;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const u32x2 b = *reinterpret_cast<const u32x2*>(row + 32 * s);  // eight codes, one per byte
    uint32_t d = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) d |= ((b[e >> 2] >> (8 * (e & 3))) & 15u) << (4 * e);
    v[s] = d;
  }
  *reinterpret_cast<u32x4*>(dst + idx * 16) = v;
  if (g == 0) dst_scale[frag * 16 + r] = scale[(tn * 16 + r) * kgroups + tk];
}

}  // namespace mi
