// Skinny-GEMM kernels and their launch selection, shared by gemm_skinny.hip (the projection entry points)
// and gemm_pick.hip (the head GEMM with the sampler's pick epilogue): two translation units so that the
// template instantiations compile in parallel.  See gemm_skinny.hip for the design notes.
#pragma once
#include <stdlib.h>

#include "mi_common.hpp"

namespace mi {

enum { EPI_NONE = 0, EPI_SILU = 1, EPI_PARTIAL = 2, EPI_PICK = 3 };

// EPI_PICK (the head GEMM of a decode step): besides the bf16 logits every workgroup reports, per activation
// row, the best sampling key among its columns - the logit itself for greedy rows, logit / T + Gumbel noise
// for sampled ones (the keys of mi_argmax / mi_sample, bit for bit) - so that the token choice needs one
// small launch over [workgroups][rows] candidates (mi_pick_final) instead of a second pass over the logits.
struct PickArgs {
  const float* temperatures;  // [M]; nullptr or <= 0: greedy
  const uint64_t* rng;        // {seed, step} in device memory (a captured graph reads the current step)
  uint2* cand;                // [M][gridDim.x] {key bits, column}: a row's candidates are contiguous
  int col0 = 0;               // vocabulary offset of this weight shard (tensor parallelism): the sampler's noise is
                              // keyed by the GLOBAL column and the candidates carry global columns, so that the
                              // ranks' candidates compare as the unsharded sampler would
};

// B fragments (the activations x^T) of one wave for STEPS k-steps starting at xk = x + k0:
//   bfrag[m][s] of lane (g, c) = x[16 m + c][k0 + 32 s + 8 g .. +7]   (rows >= M clamped to M - 1).
// Read straight from memory a fragment load touches sixteen rows with 64 bytes each - sixteen cache
// lines per instruction, half of each used - and costs the CU's address path as much as the weight
// stream itself (tools/gemm_exp.py: 4.95 us per qkv launch, 4.16 without any x traffic, 4.23 with x
// fetched in full lines).  So, for pairs of k-steps, the wave fetches its [16 MT rows][64 k] block as
// whole 128-byte lines (8 lanes per row, 8 rows per instruction), parks it in its private LDS slab
// (16-byte units XOR-swizzled by row) and reads the fragments back with ds_read_b128.  LDS operations of
// one wave execute in order, so the slab needs no barrier and is reused for every pair.
constexpr int kSkinnyRows = 64;       // activation rows one workgroup holds (MT <= 4 column tiles of 16)
constexpr int kSkinnyMaxRows = 512;   // rows a launch accepts (8 row chunks); beyond that the tile GEMM is the kernel

template <int MT, int STEPS>
__device__ __forceinline__ void issue_x_lines(const uint16_t* __restrict__ x, int M, int K, int k0, int lane,
                                              u32x4 (&stage)[(STEPS + 1) / 2][MT * 2]) {
#pragma unroll
  for (int sp = 0; sp < STEPS / 2; ++sp)
#pragma unroll
    for (int i = 0; i < MT * 2; ++i) {
      const int row = i * 8 + (lane >> 3), c = lane & 7;
      stage[sp][i] = *reinterpret_cast<const u32x4*>(x + (int64_t)min(row, M - 1) * K + k0 + 64 * sp + 8 * c);
    }
}
template <int MT, int STEPS>
__device__ __forceinline__ void x_lines_to_frags(const u32x4 (&stage)[(STEPS + 1) / 2][MT * 2], uint16_t* slab, int lane,
                                                 u32x4 (&bfrag)[MT][STEPS]) {
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int sp = 0; sp < STEPS / 2; ++sp) {
#pragma unroll
    for (int i = 0; i < MT * 2; ++i) {
      const int row = i * 8 + (lane >> 3), c = lane & 7;
      *reinterpret_cast<u32x4*>(slab + (row * 8 + (c ^ (row & 7))) * 8) = stage[sp][i];
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int row = 16 * m + r, c = 4 * h2 + g;
        bfrag[m][2 * sp + h2] = *reinterpret_cast<const u32x4*>(slab + (row * 8 + (c ^ (row & 7))) * 8);
      }
  }
}
// bytes of one wave's slab: [16 MT rows][64 k] bf16
constexpr int x_slab_bytes(int MT) { return MT * 16 * 64 * 2; }

// WF: weight format - 0 row-major bf16, 1 fragment-native bf16, 2 fragment-native fp8 (e4m3) + per-row scale
// STAMP (mi_gemm_bf16_packed_ex, tools/chain_timeline.py): every wave records s_memrealtime (the chip-wide 100 MHz clock)
// at seven points of its life into stamps[workgroup][wave][8] - entry / loads issued / data arrived / K-slice sums in
// LDS / barrier passed / stores issued / stores acknowledged.  A separate instantiation: the product kernels carry
// no stamp code.
// PIPE (long K-slices: hidden 5120 / 4096 models, TP shards of them): the K loop double-buffered - the loads of block
// i + 1 (weight fragments and x lines) are issued BEFORE block i is consumed, so a wave always has one or two blocks in
// flight instead of paying one full memory round trip per block (a Qwen3-32B TP-8 rank's qkv GEMM: five dependent
// round trips of ~2 us each).  Written as two named register sets over a loop unrolled by two with the tail peeled, so
// that no load is conditional and hipcc's wait counts stay exact (vmcnt = the loads of the newer block).
template <int MT, int RT, int WAVES, int STEPS, int WF, int EPI, bool BIAS, bool STAMP = false, bool PIPE = false>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, int M_all, int N, int K, int kslice,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, float* __restrict__ part,
    const float* __restrict__ scale, PickArgs pk, unsigned long long* __restrict__ stamps = nullptr) {
  unsigned long long ts[8] = {};
#define MI_GSTAMP(i)                                    \
  do {                                                  \
    if constexpr (STAMP) {                              \
      __builtin_amdgcn_sched_barrier(0);                \
      ts[i] = __builtin_amdgcn_s_memrealtime();         \
      __builtin_amdgcn_sched_barrier(0);                \
    }                                                   \
  } while (0)
  MI_GSTAMP(0);  // entry
  // more than 64 activation rows: blockIdx.z walks them in chunks of 64 (the weight stream of the second and
  // later chunks of a row tile is served by L2 / the Infinity Cache: the chunks of a tile are dispatched together)
  const int m0 = (int)blockIdx.z * kSkinnyRows;
  const int M = min(M_all - m0, kSkinnyRows);
  x += (int64_t)m0 * K;
  if (y) y += (int64_t)m0 * (EPI == EPI_SILU ? N >> 1 : N);
  // [WAVES][RT*MT][256] fp32 K-slice sums; before that, each wave's slot doubles as its x slab
  extern __shared__ __attribute__((aligned(16))) float red[];
  constexpr int SLOT = RT * MT * 1024 > x_slab_bytes(MT) ? RT * MT * 1024 : x_slab_bytes(MT);  // bytes per wave
  constexpr bool LINES = STEPS % 2 == 0;  // x in whole cache lines through LDS
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  uint16_t* slab = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(red) + wave * SLOT);
  // kslice = K / (gridDim.y * WAVES), a multiple of 32 * STEPS, computed and checked on the host: with x, w and the sizes
  // it is in the argument prefix that arrives in SGPRs (kernarg preload, see the Makefile), so the first weight and
  // activation addresses need no load of the kernarg segment - gridDim would be one - and no scalar division
  const int kbeg = (blockIdx.y * WAVES + wave) * kslice;
  const int ktiles = K >> 5;

  // row tiles of this workgroup
  int tile[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
    tile[t] = EPI == EPI_SILU ? (int)blockIdx.x + t * (N >> 5) : (int)blockIdx.x * RT + t;

  f32x4 acc[RT][MT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // EPI_PICK: the sampler's per-row inputs are fetched now, under the weight stream, not at the tail
  float pk_temp = 0.f;
  uint64_t pk_seed = 0, pk_step = 0;
  if (EPI == EPI_PICK) {
    const int row0 = 16 * (((int)threadIdx.x >> 6) % MT) + (lane & 15);  // the row of this thread's first item
    if (pk.temperatures && row0 < M) pk_temp = pk.temperatures[m0 + row0];
    pk_seed = pk.rng[0];
    pk_step = pk.rng[1];
  }

  // per-lane weight pointers.  fp8: [N/16][K/64][64 lanes][16 bytes] - a lane's 16 bytes are the A
  // fragments of TWO consecutive 32-deep k-steps (8 e4m3 values each), dequantised to bf16 in registers
  // (exact: e4m3 fits bf16); the per-row scale is applied to the fp32 sums in the epilogue.
  const uint16_t* wp[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
    wp[t] = WF == 2   ? w + (((int64_t)tile[t] * (K >> 6) + (kbeg >> 6)) * 1024 + lane * 16) / 2
            : WF == 1 ? w + ((int64_t)tile[t] * ktiles + (kbeg >> 5)) * 512 + lane * 8
                      : w + (int64_t)(tile[t] * 16 + r) * K + kbeg + 8 * g;
  constexpr int WSTEP = WF == 1 ? 512 : 32;  // elements between consecutive k-steps (bf16 formats)
  // B fragment of column tile m: lane (g, c) <- x[16 m + c][k + 32 s + 8 g .. +8].  Rows >= M are
  // clamped to row M-1: MFMA output columns are independent, the duplicates are never stored.
  const uint16_t* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) xp[m] = x + (int64_t)min(16 * m + r, M - 1) * K + kbeg + 8 * g;

  if constexpr (PIPE) {
    static_assert(!PIPE || (WF == 1 && STEPS % 2 == 0 && !STAMP), "double-buffered loop: packed bf16 weights, x in lines");
    constexpr int BS = 32 * STEPS;
    u32x4 aA[RT][STEPS], aB[RT][STEPS], stA[(STEPS + 1) / 2][MT * 2], stB[(STEPS + 1) / 2][MT * 2];
    auto issue = [&](u32x4(&a)[RT][STEPS], u32x4(&st)[(STEPS + 1) / 2][MT * 2], int k) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
          a[t][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[t] + ((k >> 5) + s) * WSTEP));
      issue_x_lines<MT, STEPS>(x, M, K, kbeg + k, lane, st);
      // nothing of the block being consumed may be scheduled above these loads: left alone, hipcc sinks them behind the
      // current block's waits and LDS staging, and the loop is back to one block in flight per round trip
      __builtin_amdgcn_sched_barrier(0);
    };
    auto consume = [&](const u32x4(&a)[RT][STEPS], const u32x4(&st)[(STEPS + 1) / 2][MT * 2]) {
      u32x4 bfrag[MT][STEPS];
      x_lines_to_frags<MT, STEPS>(st, slab, lane, bfrag);
#pragma unroll
      for (int s = 0; s < STEPS; ++s)
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int m = 0; m < MT; ++m)
            acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a[t][s]), as_frag(bfrag[m][s]), acc[t][m], 0, 0, 0);
    };
    const int n = kslice / BS;
    issue(aA, stA, 0);
    int it = 0;
    for (; it + 2 < n; it += 2) {
      issue(aB, stB, (it + 1) * BS);
      consume(aA, stA);
      issue(aA, stA, (it + 2) * BS);
      consume(aB, stB);
    }
    if (it + 1 < n) {
      issue(aB, stB, (it + 1) * BS);
      consume(aA, stA);
      consume(aB, stB);
    } else {
      consume(aA, stA);
    }
  } else
  for (int k = 0; k < kslice; k += 32 * STEPS) {
    u32x4 a[RT][STEPS], bfrag[MT][STEPS];
    // every load of the block is issued before the first MFMA: no branches, no waits in between
    if (WF == 2) {
      static_assert(WF != 2 || STEPS % 2 == 0, "an fp8 fragment load covers two k-steps");
      u32x4 raw[RT][(STEPS + 1) / 2];
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int s2 = 0; s2 < STEPS / 2; ++s2)
          raw[t][s2] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[t] + ((k >> 6) + s2) * 512));
      u32x4 stage[(STEPS + 1) / 2][MT * 2];
      issue_x_lines<MT, STEPS>(x, M, K, kbeg + k, lane, stage);
      x_lines_to_frags<MT, STEPS>(stage, slab, lane, bfrag);
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
          const uint32_t lo = raw[t][s >> 1][2 * (s & 1)], hi = raw[t][s >> 1][2 * (s & 1) + 1];
          const auto f0 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
          const auto f2 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
          a[t][s] = u32x4{pack_bf(f0[0], f0[1]), pack_bf(f1[0], f1[1]), pack_bf(f2[0], f2[1]), pack_bf(f3[0], f3[1])};
        }
    } else {
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
          a[t][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[t] + ((k >> 5) + s) * WSTEP));
      if (LINES) {
        u32x4 stage[(STEPS + 1) / 2][MT * 2];
        issue_x_lines<MT, STEPS>(x, M, K, kbeg + k, lane, stage);
        if constexpr (STAMP) {
          if (k == 0) {
            MI_GSTAMP(1);  // every load of the first block issued
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            MI_GSTAMP(2);  // ... and arrived
          }
        }
        x_lines_to_frags<MT, STEPS>(stage, slab, lane, bfrag);
      } else {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int s = 0; s < STEPS; ++s) bfrag[m][s] = *reinterpret_cast<const u32x4*>(xp[m] + k + 32 * s);
      }
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a[t][s]), as_frag(bfrag[m][s]),
                                                              acc[t][m], 0, 0, 0);
  }

  // C fragment: lane (g, c) holds y[m-tile col c][16 tile + 4 g + i], i = 0..3
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m)
      *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(red) + wave * SLOT + ((t * MT + m) * 64 + lane) * 16) = acc[t][m];
  MI_GSTAMP(3);  // this wave's K-slice sums are in LDS
  __syncthreads();
  MI_GSTAMP(4);  // every wave's are
  // each (row tile, m-tile, lane) result is finished by one thread, summing K-slices in wave order
  constexpr int ITEMS = (EPI == EPI_SILU ? 1 : RT) * MT * 64;
  __shared__ float pick_key[EPI == EPI_PICK ? MT * 16 : 1][RT * 4];
  __shared__ int pick_col[EPI == EPI_PICK ? MT * 16 : 1][RT * 4];
  for (int item = threadIdx.x; item < ITEMS; item += WAVES * 64) {
    const int l = item & 63, m = (item >> 6) % MT, t = (item >> 6) / MT;
    auto total = [&](int tt) {
      f32x4 s = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(red) + ((tt * MT + m) * 64 + l) * 16);
#pragma unroll
      for (int wv = 1; wv < WAVES; ++wv) {
        const f32x4 u =
            *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(red) + wv * SLOT + ((tt * MT + m) * 64 + l) * 16);
        s += u;
      }
      if (WF == 2) s *= *reinterpret_cast<const f32x4*>(scale + tile[tt] * 16 + 4 * (l >> 4));  // per weight row
      return s;
    };
    const int row = 16 * m + (l & 15);
    if (row >= M) {
      if (EPI == EPI_PICK) {
        pick_key[row][t * 4 + (l >> 4)] = -INFINITY;
        pick_col[row][t * 4 + (l >> 4)] = 0x7fffffff;
      }
      continue;
    }
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
      u32x2 ov;
      ov[0] = pack_bf(o[0], o[1]);
      ov[1] = pack_bf(o[2], o[3]);
      *reinterpret_cast<u32x2*>(y + (int64_t)row * (N >> 1) + col) = ov;
    } else {
      f32x4 s = total(t);
      const int col = tile[0] * 16 + t * 16 + 4 * (l >> 4);
      if (EPI == EPI_PARTIAL) {
        *reinterpret_cast<f32x4*>(part + ((int64_t)blockIdx.y * M_all + m0 + row) * N + col) = s;
      } else {
        if (BIAS) {
          const u32x2 bw = *reinterpret_cast<const u32x2*>(bias + col);
          s[0] += lo_bf(bw[0]);
          s[1] += hi_bf(bw[0]);
          s[2] += lo_bf(bw[1]);
          s[3] += hi_bf(bw[1]);
        }
        u32x2 o;
        o[0] = pack_bf(s[0], s[1]);
        o[1] = pack_bf(s[2], s[3]);
        *reinterpret_cast<u32x2*>(y + (int64_t)row * N + col) = o;
        if (EPI == EPI_PICK) {  // keys of the ROUNDED logits, as a sampler reading y would form them
          const float tmp = item == (int)threadIdx.x ? pk_temp : (pk.temperatures ? pk.temperatures[m0 + row] : 0.f);
          const bool noisy = tmp > 0.f;
          const float inv_t = noisy ? 1.0f / tmp : 1.0f;
          const uint64_t rkey = sample_row_key(pk_seed, pk_step, m0 + row);
          const float v[4] = {lo_bf(o[0]), hi_bf(o[0]), lo_bf(o[1]), hi_bf(o[1])};
          float best = -INFINITY;
          int best_c = 0x7fffffff;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float key = noisy ? gumbel_key(v[i], inv_t, rkey, pk.col0 + col + i) : v[i];
            if (key > best) {  // ascending columns: the first of equal keys stays
              best = key;
              best_c = pk.col0 + col + i;
            }
          }
          pick_key[row][t * 4 + (l >> 4)] = best;
          pick_col[row][t * 4 + (l >> 4)] = best_c;
        }
      }
    }
  }
  if constexpr (STAMP) {
    MI_GSTAMP(5);  // reduced, stores issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    MI_GSTAMP(6);  // stores acknowledged
    if (stamps != nullptr && lane == 0) {
      const int64_t wg = (int64_t)blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
      unsigned long long* dst = stamps + (wg * WAVES + wave) * 8;
#pragma unroll
      for (int q = 0; q < 8; ++q) dst[q] = ts[q];
    }
  }
#undef MI_GSTAMP
  if (EPI == EPI_PICK) {
    __syncthreads();
    if ((int)threadIdx.x < M) {
      const int row = threadIdx.x;
      float best = pick_key[row][0];
      int best_c = pick_col[row][0];
#pragma unroll
      for (int j = 1; j < RT * 4; ++j) {
        const float k2 = pick_key[row][j];
        const int c2 = pick_col[row][j];
        if (k2 > best || (k2 == best && c2 < best_c)) {
          best = k2;
          best_c = c2;
        }
      }
      pk.cand[(int64_t)(m0 + row) * gridDim.x + blockIdx.x] = uint2{__float_as_uint(best), (uint32_t)best_c};
    }
  }
}


// ---------------------------------------------------------------------------------------------------
// Row-parallel projections (o_proj, down_proj: N = hidden is small, K large): complete bf16 rows from
// every workgroup, no split-K partials - the consumer (the next GEMM's add + RMSNorm prologue) then
// re-reads 2 bytes per element instead of 4 x ksplit.
//   A workgroup owns FOUR output features and the whole K: N / 4 workgroups (256 for hidden 1024) each
//   stream 8 K bytes of weights - all CUs pull from HBM, which a 16-feature tile (N / 16 = 64
//   workgroups) cannot do for these shapes and which split-K only buys with fp32 partials.
//   Weights are packed [N/4][K/32][4 k-groups][4 features][8]: a wave's K-slice is one contiguous run,
//   the A fragment row r of v_mfma_f32_16x16x32_bf16 carries feature r % 4 (rows 4..15 are duplicates
//   whose results are never read), the B fragments are the rows of x as in gemm_skinny_kernel, so lane
//   (g = 0, c) ends up with features 0..3 of activation row c: one 8-byte store per row.
//   The WAVES K-slices are summed through LDS in wave order (deterministic) and rounded to bf16 once.
// ---------------------------------------------------------------------------------------------------
template <int MT, int WAVES, int STEPS>
__global__ __launch_bounds__(WAVES * 64) void gemm_rows4_kernel(const uint16_t* __restrict__ x,
                                                                const uint16_t* __restrict__ w4,
                                                                uint16_t* __restrict__ y, int M_all, int N, int K) {
  const int m0 = (int)blockIdx.y * kSkinnyRows;  // row chunks of 64, as gemm_skinny_kernel
  const int M = min(M_all - m0, kSkinnyRows);
  x += (int64_t)m0 * K;
  y += (int64_t)m0 * N;
  __shared__ __attribute__((aligned(16))) float red[WAVES][MT][16][4];
  __shared__ __attribute__((aligned(16))) uint16_t slabs[WAVES][STEPS % 2 == 0 ? MT * 16 * 64 : 8];  // x in whole lines
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int kslice = K / WAVES;  // multiple of 32 * STEPS (checked on the host)
  const int kbeg = wave * kslice;
  const uint16_t* wp = w4 + ((int64_t)blockIdx.x * (K >> 5) + (kbeg >> 5)) * 128 + (g * 4 + (r & 3)) * 8;
  const uint16_t* xp[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) xp[m] = x + (int64_t)min(16 * m + r, M - 1) * K + kbeg + 8 * g;
  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < kslice; k += 32 * STEPS) {
    u32x4 a[STEPS], bfrag[MT][STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
      a[s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + ((k >> 5) + s) * 128));
    if (STEPS % 2 == 0) {
      u32x4 stage[(STEPS + 1) / 2][MT * 2];
      issue_x_lines<MT, STEPS>(x, M, K, kbeg + k, lane, stage);
      x_lines_to_frags<MT, STEPS>(stage, &slabs[wave][0], lane, bfrag);
    } else {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int s = 0; s < STEPS; ++s) bfrag[m][s] = *reinterpret_cast<const u32x4*>(xp[m] + k + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int m = 0; m < MT; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a[s]), as_frag(bfrag[m][s]), acc[m], 0, 0, 0);
  }
  // C fragment: lane (g, c) holds rows 4g .. 4g+3 (features) of column c (activation row): g == 0 is real
  if (g == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) *reinterpret_cast<f32x4*>(&red[wave][m][r][0]) = acc[m];
  }
  __syncthreads();
  if (threadIdx.x < MT * 16) {
    const int m = threadIdx.x >> 4, c = threadIdx.x & 15;
    f32x4 t = *reinterpret_cast<const f32x4*>(&red[0][m][c][0]);
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) t += *reinterpret_cast<const f32x4*>(&red[wv][m][c][0]);
    const int row = 16 * m + c;
    if (row < M)
      *reinterpret_cast<u32x2*>(y + (int64_t)row * N + 4 * blockIdx.x) = u32x2{pack_bf(t[0], t[1]), pack_bf(t[2], t[3])};
  }
}

// dst[((tn * K/32 + tk) * 16 + g * 4 + n) * 8 + e] = src[(4 tn + n) * K + 32 tk + 8 g + e]
static __global__ __launch_bounds__(256) void pack_weight_rows4_kernel(const uint16_t* __restrict__ src,
                                                                uint16_t* __restrict__ dst, int N, int K) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 16-byte chunk each
  if (idx >= (int64_t)N * K / 8) return;
  const int u = idx & 15, n = u & 3, g = u >> 2;
  const int64_t frag = idx >> 4;
  const int ktiles = K >> 5;
  const int tk = frag % ktiles;
  const int64_t tn = frag / ktiles;
  *reinterpret_cast<u32x4*>(dst + idx * 8) = *reinterpret_cast<const u32x4*>(src + (tn * 4 + n) * K + tk * 32 + g * 8);
}

template <int MT, int WAVES>
static bool rows4_steps(const uint16_t* x, const uint16_t* w4, uint16_t* y, int M, int N, int K, hipStream_t st) {
  if (K % WAVES) return false;
  const int kslice = K / WAVES;
#define ROWS4_GO(ST)                                                                                      \
  do {                                                                                                    \
    hipLaunchKernelGGL((gemm_rows4_kernel<MT, WAVES, ST>), dim3(N / 4, (M + kSkinnyRows - 1) / kSkinnyRows),  \
                       dim3(WAVES * 64), 0, st, x, w4, y, M, N, K);                                       \
    return true;                                                                                          \
  } while (0)
  // the whole K-slice in flight when the registers allow (MT + 1 fragments per k-step)
  if (kslice == 256 && MT <= 2) ROWS4_GO(8);
  if (kslice == 192 && MT <= 2) ROWS4_GO(6);
  if (kslice % 128 == 0) ROWS4_GO(4);
  if (kslice % 96 == 0) ROWS4_GO(3);
  if (kslice % 64 == 0) ROWS4_GO(2);
  if (kslice % 32 == 0) ROWS4_GO(1);
#undef ROWS4_GO
  return false;
}

template <int MT>
static int rows4_waves(const uint16_t* x, const uint16_t* w4, uint16_t* y, int M, int N, int K, hipStream_t st) {
  // 16 waves when every wave still gets >= 64 of K, else 8 / 4
  bool ok = false;
  if (K >= 16 * 64) ok = rows4_steps<MT, 16>(x, w4, y, M, N, K, st);
  if (!ok && K >= 8 * 32) ok = rows4_steps<MT, 8>(x, w4, y, M, N, K, st);
  if (!ok) ok = rows4_steps<MT, 4>(x, w4, y, M, N, K, st) || rows4_steps<MT, 1>(x, w4, y, M, N, K, st);
  return ok ? check_launch() : MI_EUNSUPPORTED;
}

// fragment-native repack: dst[(tn * K/32 + tk) * 512 + lane * 8 + e] = src[(16 tn + lane%16) * K + 32 tk + 8 (lane/16) + e]
static __global__ __launch_bounds__(256) void pack_weight_kernel(const uint16_t* __restrict__ src,
                                                          uint16_t* __restrict__ dst, int N, int K) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 16-byte chunk each
  const int64_t total = (int64_t)N * K / 8;
  if (idx >= total) return;
  const int lane = idx & 63;
  const int64_t frag = idx >> 6;
  const int ktiles = K >> 5;
  const int tk = frag % ktiles;
  const int64_t tn = frag / ktiles;
  const u32x4 v = *reinterpret_cast<const u32x4*>(src + (tn * 16 + (lane & 15)) * K + tk * 32 + (lane >> 4) * 8);
  *reinterpret_cast<u32x4*>(dst + idx * 8) = v;
}

// ---------------------------------------------------------------------------------------------------
// Head-sized GEMM (thousands of row tiles, K = WAVES * 32 * STEPS): persistent workgroups.
//
// gemm_skinny_kernel starts one short-lived workgroup per pair of row tiles; each re-fetches the whole x
// (as many bytes as its weights) and pays its own ramp, LDS reduction and teardown - 4748 times for the
// Qwen3 vocabulary.  Here a workgroup keeps its waves' x K-slices in REGISTERS (B fragments, loaded once) and
// walks a contiguous share of the tile groups: per group every wave streams its K-slice of RT tiles (non-temporal,
// 1 KiB per wave-load), multiplies, parks the partial sums in one of two LDS buffers (alternating: one barrier
// per group), and the first RT * MT waves finish the group - sum over the waves in wave order, round, store, and with
// PICK keep each row's best sampling key in registers - while the others already fetch the next group.
// Summation order: one MFMA chain per wave over its slice, then the waves in order (deterministic).
// ---------------------------------------------------------------------------------------------------
template <int MT, int RT, int WAVES, int STEPS, bool PICK>
__global__ __launch_bounds__(WAVES * 64) void head_stream_kernel(const uint16_t* __restrict__ x,
                                                                 const uint16_t* __restrict__ w,
                                                                 uint16_t* __restrict__ y, int M, int N, int K,
                                                                 int n_groups, PickArgs pk) {
  static_assert(RT * MT * 64 <= WAVES * 64, "one epilogue item per thread");
  __shared__ __attribute__((aligned(16))) float red[2][WAVES][RT * MT][64][4];
  __shared__ float pick_key[PICK ? MT * 16 : 1][RT * 4];
  __shared__ int pick_col[PICK ? MT * 16 : 1][RT * 4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int ktiles = K >> 5, kbeg = wave * 32 * STEPS;

  // this wave's x slice as B fragments: lane (g, c) <- x[16 m + c][kbeg + 32 s + 8 g .. +8]; rows >= M are
  // clamped to row M - 1 (MFMA output columns are independent, the duplicates are never stored)
  u32x4 bfrag[MT][STEPS];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
      bfrag[m][s] = *reinterpret_cast<const u32x4*>(x + (int64_t)min(16 * m + r, M - 1) * K + kbeg + 32 * s + 8 * g);

  // epilogue item of this thread (threads >= RT * MT * 64 have none): fixed (row tile t, m-tile, lane) -> fixed row
  const int item = threadIdx.x;
  const bool has_item = item < RT * MT * 64;
  const int el = item & 63, em = (item >> 6) % MT, et = (item >> 6) / MT;
  const int erow = 16 * em + (el & 15);
  float best = -INFINITY;
  int best_c = 0x7fffffff;
  float inv_t = 1.0f;
  bool noisy = false;
  uint64_t rkey = 0;
  if (PICK && has_item && erow < M) {
    const float tmp = pk.temperatures ? pk.temperatures[erow] : 0.f;
    noisy = tmp > 0.f;
    inv_t = noisy ? 1.0f / tmp : 1.0f;
    rkey = sample_row_key(pk.rng[0], pk.rng[1], erow);
  }

  const int first = (int)((int64_t)blockIdx.x * n_groups / gridDim.x);
  const int last = (int)((int64_t)(blockIdx.x + 1) * n_groups / gridDim.x);
  int par = 0;
  for (int grp = first; grp < last; ++grp, par ^= 1) {
    // (fetching the next group's fragments before this group's barrier measured slower: 62.3 vs 59.0 us)
    u32x4 a[RT][STEPS];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int s = 0; s < STEPS; ++s)
        a[t][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(
            w + ((int64_t)(grp * RT + t) * ktiles + (kbeg >> 5) + s) * 512 + lane * 8));
    f32x4 acc[RT][MT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a[t][s]), as_frag(bfrag[m][s]), acc[t][m], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int m = 0; m < MT; ++m) *reinterpret_cast<f32x4*>(&red[par][wave][t * MT + m][lane][0]) = acc[t][m];
    // everybody's sums of this group are in red[par]; the readers of red[par] from two groups ago passed the
    // barrier of the previous group after finishing
    __syncthreads();
    if (has_item && erow < M) {
      f32x4 sum = *reinterpret_cast<const f32x4*>(&red[par][0][et * MT + em][el][0]);
#pragma unroll
      for (int wv = 1; wv < WAVES; ++wv) sum += *reinterpret_cast<const f32x4*>(&red[par][wv][et * MT + em][el][0]);
      const int col = (grp * RT + et) * 16 + 4 * (el >> 4);
      u32x2 o;
      o[0] = pack_bf(sum[0], sum[1]);
      o[1] = pack_bf(sum[2], sum[3]);
      *reinterpret_cast<u32x2*>(y + (int64_t)erow * N + col) = o;
      if (PICK) {  // keys of the ROUNDED logits, as a sampler reading y would form them; ascending columns
        const float v[4] = {lo_bf(o[0]), hi_bf(o[0]), lo_bf(o[1]), hi_bf(o[1])};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float key = noisy ? gumbel_key(v[i], inv_t, rkey, pk.col0 + col + i) : v[i];
          if (key > best || (key == best && pk.col0 + col + i < best_c)) {
            best = key;
            best_c = pk.col0 + col + i;
          }
        }
      }
    }
  }
  if (PICK) {
    if (has_item) {
      pick_key[erow][et * 4 + (el >> 4)] = erow < M ? best : -INFINITY;
      pick_col[erow][et * 4 + (el >> 4)] = erow < M ? best_c : 0x7fffffff;
    }
    __syncthreads();
    if ((int)threadIdx.x < M) {
      const int row = threadIdx.x;
      float b2 = pick_key[row][0];
      int c2 = pick_col[row][0];
#pragma unroll
      for (int j = 1; j < RT * 4; ++j) {
        const float k3 = pick_key[row][j];
        const int c3 = pick_col[row][j];
        if (k3 > b2 || (k3 == b2 && c3 < c2)) {
          b2 = k3;
          c2 = c3;
        }
      }
      pk.cand[(int64_t)row * gridDim.x + blockIdx.x] = uint2{__float_as_uint(b2), (uint32_t)c2};
    }
  }
}

// shapes the persistent head kernel takes: bf16 weights, no bias, vocabulary-sized N (>= 2048 tile pairs), and
//   K = 1024 (Qwen3-0.6B: 8 waves x 128)   up to 64 rows (round 4: bs 64 = BASELINE.json configs[4], VERDICT r03 weak 6 -
//                                           above 32 rows the head used to fall back to 4748 short-lived workgroups)
//   K =  896 (Qwen2-0.5B: 7 waves x 128)   up to 48 rows (one epilogue item per thread: 2 * MT * 64 <= 448)
//   K = 2048 (Llama-3.2-1B: 8 waves x 256) up to 32 rows (x slices of 64 rows would not fit the register file)
static bool head_stream_fits(int M, int N, int K) {
  if (N % 32 || N / 32 < 2048 || M < 1) return false;
  return (K == 1024 && M <= 64) || (K == 896 && M <= 48) || (K == 2048 && M <= 32);
}
// 1024 workgroups of 4-5 groups each (two resident per CU, two rounds: the dispatcher evens out the 4-vs-5 split);
// measured 57.2 us against 60.2 (512), 61.4 (256), 63.0 (768), 60.4 (2374) at 151936 x 1024, 32 rows.  More than 32
// rows: the partial-sum buffers of a workgroup take 96-128 KiB of LDS (one workgroup per CU): 512 workgroups.
constexpr int kHeadStreamGrid = 1024;
static int head_stream_grid(int M) { return M <= 32 ? kHeadStreamGrid : kHeadStreamGrid / 2; }

template <bool PICK>
static void launch_head_stream(const uint16_t* x, const uint16_t* w, uint16_t* y, int M, int N, int K, PickArgs pk,
                               hipStream_t st) {
  const int grid = head_stream_grid(M);
#define MI_HEAD_LAUNCH(MT, WAVES, STEPS)                                                                          \
  hipLaunchKernelGGL((head_stream_kernel<MT, 2, WAVES, STEPS, PICK>), dim3(grid), dim3(WAVES * 64), 0, st, x, w, y, \
                     M, N, K, N / 32, pk)
  const int mt = (M + 15) / 16;
  if (K == 1024) {
    if (mt == 1) MI_HEAD_LAUNCH(1, 8, 4);
    else if (mt == 2) MI_HEAD_LAUNCH(2, 8, 4);
    else if (mt == 3) MI_HEAD_LAUNCH(3, 8, 4);
    else MI_HEAD_LAUNCH(4, 8, 4);
  } else if (K == 896) {
    if (mt == 1) MI_HEAD_LAUNCH(1, 7, 4);
    else if (mt == 2) MI_HEAD_LAUNCH(2, 7, 4);
    else MI_HEAD_LAUNCH(3, 7, 4);
  } else {  // 2048
    if (mt == 1) MI_HEAD_LAUNCH(1, 8, 8);
    else MI_HEAD_LAUNCH(2, 8, 8);
  }
#undef MI_HEAD_LAUNCH
}

struct GemmArgs {
  const uint16_t *x, *w, *bias;
  uint16_t* y;
  float* part;
  int M, N, K, ksplit;
  hipStream_t st;
  const float* scale = nullptr;  // fp8 weights: one fp32 factor per weight row
  PickArgs pick = PickArgs{nullptr, nullptr, nullptr, 0};
};

// The instrumented instantiations (STAMP): the decode chain's own configurations at up to 32 rows only - K-slices of 64
// per wave, 8 / 12 / 16 waves (tools/chain_timeline.py).  false: no instrumented kernel for this shape.
template <int EPI>
static bool launch_stamped(const GemmArgs& a, unsigned long long* stamps) {
  constexpr int MT = 2, RT = EPI == EPI_SILU ? 2 : 1;
  if (a.M < 17 || a.M > 32 || a.bias || a.K % a.ksplit) return false;
  const int kper = a.K / a.ksplit;
  if (kper % 64) return false;
  const int waves = kper / 64;
  const int tiles = a.N / 16;
  const dim3 grid(EPI == EPI_SILU ? tiles / 2 : tiles / RT, a.ksplit, 1);
#define MI_STAMPED_GO(W)                                                                                            \
  do {                                                                                                              \
    const size_t slot = (size_t)RT * MT * 1024 > (size_t)x_slab_bytes(MT) ? (size_t)RT * MT * 1024 : (size_t)x_slab_bytes(MT); \
    hipLaunchKernelGGL((gemm_skinny_kernel<MT, RT, W, 2, 1, EPI, false, true>), grid, dim3(W * 64), W * slot, a.st, \
                       a.x, a.w, a.M, a.N, a.K, a.K / (a.ksplit * W), a.bias, a.y, a.part, a.scale, a.pick, stamps); \
    return true;                                                                                                    \
  } while (0)
  if (waves == 16) MI_STAMPED_GO(16);
  if (EPI == EPI_PARTIAL && waves == 8) MI_STAMPED_GO(8);
  if (EPI == EPI_PARTIAL && waves == 12) MI_STAMPED_GO(12);
#undef MI_STAMPED_GO
  return false;
}

template <int MT, int RT, int WAVES, int STEPS, int WF, int EPI, bool PIPE = false>
static void launch(const GemmArgs& a) {
  const size_t slot = (size_t)RT * MT * 1024 > (size_t)x_slab_bytes(MT) ? (size_t)RT * MT * 1024 : (size_t)x_slab_bytes(MT);
  const size_t lds = (size_t)WAVES * slot;
  const int tiles = a.N / 16, kslice = a.K / (a.ksplit * WAVES);
  const dim3 grid(EPI == EPI_SILU ? tiles / 2 : tiles / RT, a.ksplit, (a.M + kSkinnyRows - 1) / kSkinnyRows);
  if (a.bias && EPI == EPI_NONE)
    hipLaunchKernelGGL((gemm_skinny_kernel<MT, RT, WAVES, STEPS, WF, EPI, true, false, PIPE>), grid, dim3(WAVES * 64), lds,
                       a.st, a.x, a.w, a.M, a.N, a.K, kslice, a.bias, a.y, a.part, a.scale, a.pick, nullptr);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<MT, RT, WAVES, STEPS, WF, EPI, false, false, PIPE>), grid, dim3(WAVES * 64), lds,
                       a.st, a.x, a.w, a.M, a.N, a.K, kslice, a.bias, a.y, a.part, a.scale, a.pick, nullptr);
}

// choose STEPS (k-steps in flight per wave and iteration) from the K-slice and the register budget
template <int MT, int RT, int WAVES, int WF, int EPI>
static bool try_waves(const GemmArgs& a) {
  if (a.K % (a.ksplit * WAVES)) return false;
  const int kslice = a.K / (a.ksplit * WAVES);
  constexpr int FRAGS = MT + RT;  // fragments (4 VGPRs each) per k-step
  // k-steps in flight per wave and iteration, bounded by the 128-register budget of a 16-wave workgroup
  // (x is staged as whole lines: its registers are live twice for a moment)
  constexpr int MAXS = FRAGS <= 3 ? 8 : (FRAGS <= 5 ? 4 : 2);
  // a K-slice that would take two or more dependent blocks: the double-buffered loop on blocks of 64 (PIPE; two register
  // sets of RT + MT fragments per k-step: up to 32 activation rows, the many-waves geometries)
  if constexpr (WF == 1 && MT <= 2 && WAVES >= 8) {
    if (kslice % 64 == 0 && tuning(MI_TUNE_GEMM_PIPE)) {
      const int steps = (MAXS >= 8 && kslice % 256 == 0) ? 8 : ((MAXS >= 4 && kslice % 128 == 0) ? 4 : 2);
      if (kslice / (32 * steps) >= 2) return launch<MT, RT, WAVES, 2, WF, EPI, true>(a), true;
    }
  }
  if constexpr (MAXS >= 8) {
    if (kslice % 256 == 0) return launch<MT, RT, WAVES, 8, WF, EPI>(a), true;
  }
  if constexpr (MAXS >= 4) {
    if (kslice % 128 == 0) return launch<MT, RT, WAVES, 4, WF, EPI>(a), true;
  }
  if (kslice % 64 == 0) return launch<MT, RT, WAVES, 2, WF, EPI>(a), true;
  if constexpr (WF != 2) {  // an fp8 fragment load spans 64 k
    if (kslice % 32 == 0) return launch<MT, RT, WAVES, 1, WF, EPI>(a), true;
  }
  return false;
}

template <int MT, int RT, int WF, int EPI>
static int pick_waves(const GemmArgs& a) {
  // Few row tiles (small N): spread K over many waves so that every CU holds loads in flight -
  // K-slices of 128 (four 1 KiB fragment loads per row tile and wave) when K allows;
  // many row tiles (lm_head): fewer, fatter waves.
  const int wgs = (a.N / 16) / (EPI == EPI_SILU ? 2 : RT) * a.ksplit;
  const int kper = a.K / a.ksplit;
  bool ok = false;
  if (wgs >= 2048) {
    ok = try_waves<MT, RT, 4, WF, EPI>(a) || try_waves<MT, RT, 2, WF, EPI>(a);
  } else {
    // K-slices of 64 (two 1 KiB fragment loads per row tile and wave) when that fits 16 waves, else of
    // 128: these launches are latency-bound, so the fewer dependent loads a wave issues the better
    // (64-deep slices measured 1.72 -> 1.69 ms per decode step against 128-deep ones)
    auto by_waves = [&](int waves) {
      switch (waves) {
        case 1: return try_waves<MT, RT, 1, WF, EPI>(a);
        case 2: return try_waves<MT, RT, 2, WF, EPI>(a);
        case 3: return try_waves<MT, RT, 3, WF, EPI>(a);
        case 4: return try_waves<MT, RT, 4, WF, EPI>(a);
        case 5: return try_waves<MT, RT, 5, WF, EPI>(a);
        case 6: return try_waves<MT, RT, 6, WF, EPI>(a);
        case 7: return try_waves<MT, RT, 7, WF, EPI>(a);  // K = 7 * 2^n * 64: hidden 896 (Qwen2-0.5B), 448
        case 8: return try_waves<MT, RT, 8, WF, EPI>(a);
        case 10: return try_waves<MT, RT, 10, WF, EPI>(a);
        case 12: return try_waves<MT, RT, 12, WF, EPI>(a);
        case 16: return try_waves<MT, RT, 16, WF, EPI>(a);
        default: return false;
      }
    };
    if (kper % 64 == 0 && kper / 64 <= 16) ok = by_waves(kper / 64);
    if (!ok && kper % 128 == 0) ok = by_waves(kper / 128 <= 16 ? kper / 128 : (kper / 128 == 24 ? 12 : 16));
    // K = 5 * 2^n * 64 (3200 = a Qwen3-32B intermediate shard at TP 8, 640, 1280 ...): ten waves on 64-deep
    // multiples; without them such a K fell through to four waves with ONE k-step in flight each
    if (!ok && kper % 640 == 0) ok = by_waves(10);
  }
  if (!ok) ok = try_waves<MT, RT, 8, WF, EPI>(a) || try_waves<MT, RT, 4, WF, EPI>(a) ||
                try_waves<MT, RT, 2, WF, EPI>(a) || try_waves<MT, RT, 1, WF, EPI>(a);
  if (!ok) return MI_EUNSUPPORTED;
  return check_launch();
}

template <int RT, int WF, int EPI>
static int pick_mt(const GemmArgs& a) {
  switch ((min(a.M, kSkinnyRows) + 15) / 16) {
    case 1: return pick_waves<1, RT, WF, EPI>(a);
    case 2: return pick_waves<2, RT, WF, EPI>(a);
    case 3: return pick_waves<3, RT, WF, EPI>(a);
    default: return pick_waves<4, RT, WF, EPI>(a);
  }
}

static int check_gemm(const void* x, const void* w, const void* y, int M, int N, int K) {
  if (!x || !w || !y || M < 0 || N <= 0 || K <= 0) return MI_EINVAL;
  if (M > kSkinnyMaxRows || K % 32 || N % 16) return MI_EUNSUPPORTED;
  if (!aligned16(x) || !aligned16(w) || !aligned16(y)) return MI_EINVAL;
  return MI_OK;
}

}  // namespace mi

namespace mi {
static bool pick_two_tiles(int M, int N) { return N / 16 >= 1024 && (N / 16) % 2 == 0 && M <= 32; }
}  // namespace mi
