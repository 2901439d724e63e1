// Prefill over the fp8 (e4m3) paged KV cache: causal GQA attention that reads the e4m3 tiles directly, and the
// prefill-sized fused k-norm + RoPE + quantising store.  With these two launches an fp8 prefill layer no longer runs
// q-norm, k-norm, RoPE, mi_kv_store_fp8, mi_kv_fp8_expand and mi_paged_attn_prefill as six launches over a bf16 scratch.
//
// Attention.  The work split of the bf16 prefill kernel (paged_attn.hip): a four-wave workgroup owns 128 MFMA columns
// (128/G query tokens x G heads) of one (sequence, kv head), walks the 32-key chunks once, workgroup ids dealt so that
// all query blocks of a pair land on one XCD, the heaviest query blocks first.  What differs is everything between the
// cache and the MFMA operands:
//   feed     a chunk is K0 | K1 | V0 | V1 = 4 x 2112 bytes (16 KiB in bf16).  Wave w copies piece w as stored with THREE
//            buffer_load ... lds per chunk: two of 1 KiB (the e4m3 bytes) and one of 64 bytes by lanes 0 .. 3 (the
//            tile's 16 scales, which follow the data: they arrive with the tile, by DMA, in the same slot).  The loop's
//            wait is therefore vmcnt(6): all but the two newest chunks of this wave.
//   ring     FOUR slots of 8448 bytes = 33 KiB: chunk c is computed while c + 1, c + 2 and c + 3 are landing.  The ring
//            cannot be shallower than the 32 KiB the output transposition needs, and the kernel's registers allow two
//            workgroups per CU, not three, so the room the smaller chunks leave goes into depth.
//   K        S^T[32 keys][32 cols] = K . Q^T on v_mfma_f32_32x32x16_bf16.  Lane (hi, n) needs K[token n][16 kk + 8 hi ..
//            + 7]: in the fp8 layout 8 contiguous bytes whose neighbours are the same lane's operand for dims + 32, so
//            one ds_read_b128 (16-byte lane stride: every quarter wave reads 256 contiguous bytes, conflict-free) feeds
//            the k-steps 4 i + b and 4 i + 2 + b; dq8 turns each half into a fragment (exact).
//   V        O^T[128 dims][32 cols] += V^T . P^T.  The score registers of lane half `hi` hold the keys 16 s + 4 hi + r
//            and 16 s + 8 + 4 hi + r of tile s; a V dword holds tokens 4 g .. 4 g + 3 of one dim, so the A operand of
//            k-step s is the dwords of token groups hi and 2 + hi of tile s, 512 bytes apart, and P never moves
//            between lanes.
//   scales   both are powers of two, both exact: K's multiplies the fp32 score of its key (folded into the softmax's
//            multiply-add with scale * log2 e), V's the probability before its rounding to bf16; the running sum takes
//            the unscaled exponentials.  A lane reads the scales of its sixteen keys as four broadcast ds_read_b128 each.
//   softmax  the bf16 kernel's product form (deferred maximum, the lane's sum of exponentials as the test), P as one
//            bf16 per key.  MI_TUNE_PREFILL_P_SPLIT does not apply here.
//   masking  a masked key's score is -inf before the exponential, so its probability is exactly 0 whatever finite
//            bytes and scales sit in the tile behind it (0 x finite = 0 in the second product as well).
#include <limits.h>

#include "mi_common.hpp"
#include "kv_store.hpp"
#include "kv8_common.hpp"
#include "prefill_common.hpp"

namespace mi {

template <int G, bool FUSE_Q>
__global__ __launch_bounds__(256) void paged_attn_prefill_fp8kv_kernel(
    const uint16_t* __restrict__ q, int64_t q_stride, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const int32_t* __restrict__ block_table, int table_stride, const int32_t* __restrict__ cu_q,
    const int32_t* __restrict__ kv_lens, uint16_t* __restrict__ out, int n_q_heads, int n_kv_heads, int tpb,
    int tpb_shift, float scale_log2e, int n_qblocks, int n_pairs, QPrep qp) {
  constexpr int D = 128;
  constexpr int TQ = 32 / G;      // query tokens per wave
  constexpr int TQ_WG = 4 * TQ;   // per workgroup
  constexpr int NBUF = 4;         // LDS ring: chunk c is computed while c + 1 .. c + 3 are landing
  __shared__ __attribute__((aligned(16))) uint8_t stage[NBUF][4][KV8_TILE];  // [slot][K0, K1, V0, V1][tile as stored]
  static_assert(sizeof(stage) >= 4 * 32 * D * 2, "the output transposition needs 8 KiB per wave");

  // (the bf16 kernel's deal: all query blocks of a (sequence, kv head) pair get ids that are equal mod 8 - one XCD)
  const int pair = ((int)blockIdx.x / (8 * n_qblocks)) * 8 + ((int)blockIdx.x & 7);
  const int qblock = ((int)blockIdx.x >> 3) % n_qblocks;
  if (pair >= n_pairs) return;
  const int seq = pair / n_kv_heads, h = pair % n_kv_heads;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5, n = lane & 31;
  const int q_start = cu_q[seq];
  const int q_len = cu_q[seq + 1] - q_start;
  const int kv_len = kv_lens[seq];
  const int wg_qt0 = (n_qblocks - 1 - qblock) * TQ_WG;  // heaviest (latest) query blocks are dispatched first
  if (wg_qt0 >= q_len) return;                          // uniform for the workgroup
  const int shift = kv_len - q_len;
  const int wg_last_pos = shift + min(wg_qt0 + TQ_WG, q_len) - 1;
  if (wg_last_pos < 0) return;  // kv_len < q_len is outside the contract: no key, and no table entry, is touched
  const int wg_chunks = (wg_last_pos + 32) >> 5, wg_tiles = (wg_last_pos + 16) >> 4;

  const int qt0 = wg_qt0 + wave * TQ;
  const bool wave_on = qt0 < q_len;
  const int my_qt = qt0 + n / G, hn = n % G;
  const bool valid = wave_on && my_qt < q_len;
  const int limit = valid ? shift + my_qt + 1 : 1;  // keys [0, limit) are visible to this lane's column
  const int wave_chunks = wave_on ? (shift + min(qt0 + TQ, q_len) - 1 + 32) >> 5 : 0;
  const int limit_all = wave_on && qt0 + TQ <= q_len ? shift + qt0 + 1 : 0;  // earliest column of a full block

  bf16x8 Q[8];  // B operand of S^T = K . Q^T: column n, dims 16 kk + 8 hi .. +7
  {
    const int row = valid ? my_qt : wg_qt0;  // invalid columns read a valid row and are zeroed
    const uint16_t* qrow = q + (int64_t)(q_start + row) * q_stride + (int64_t)(h * G + hn) * D + 8 * hi;
    if constexpr (FUSE_Q) {
      float xq[8][8];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) load16(qrow + 16 * kk, xq[kk]);
      head_rmsnorm_rope_q32(xq, qp.q_w, qp.cos_sin + qp.positions[q_start + row] * 128, hi, qp.eps);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        u32x4 v = pack16(xq[kk]);
        if (!valid) v = u32x4{0, 0, 0, 0};
        Q[kk] = as_frag(v);
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        u32x4 v = *reinterpret_cast<const u32x4*>(qrow + 16 * kk);
        if (!valid) v = u32x4{0, 0, 0, 0};
        Q[kk] = as_frag(v);
      }
    }
  }
  float m = -INFINITY, l = 0.f;  // running reference point (log2 domain) and this lane's share of the running sum
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

  // ---- the request side: wave w fetches piece w (K0, K1, V0, V1) of every chunk, the tile's address on the scalar unit
  const int32_t* table_row = block_table + (int64_t)seq * table_stride;
  const int piece = wave, odd = piece & 1;
  const uint8_t* const cache_h = ((piece & 2) ? vc : kc) + (int64_t)h * tpb * KV8_TILE;  // (wave-uniform)
  const int block_bytes = n_kv_heads * tpb * KV8_TILE;                                   // (< 2^31: checked by the host)
  const uint32_t lane16 = lane * 16;
  // request r fetches tile min(2 r + odd, t_max) - past the end the last chunk again, into its own slot, which keeps
  // the vmcnt arithmetic uniform - from block-table entry rq_bi, tile rq_in of that block, into ring slot rq_slot
  const int r_last = wg_chunks - 1, t_max = min(2 * r_last + odd, wg_tiles - 1);
  auto request = [&](int slot, int blk, int in_block) __attribute__((always_inline)) {
    const uint8_t* base = cache_h + (int64_t)blk * block_bytes + in_block * KV8_TILE;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, KV8_TILE, 0x00020000);
    uint8_t* dst = &stage[0][piece][0] + slot * (4 * KV8_TILE);
    // (the pieces of 1 KiB as SCALAR offsets: an instruction's immediate offset would move the LDS destination too)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, lane16, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + 1024), 16, lane16, 1024, 0, 0);
    if (lane < 4)  // the 64 bytes of scales: lane i's 16 bytes land at dst + 2048 + 16 i; one more vmcnt event per wave
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + KV8_DATA), 16, lane16,
                                               KV8_DATA, 0, 0);
  };
  auto locate = [&](int t, int& bi, int& in_block) {
    bi = tpb_shift >= 0 ? t >> tpb_shift : t / tpb;
    in_block = t - bi * tpb;
  };
  // The loop's wait is a COUNT (vmcnt(6) = all but this wave's six newest vector-memory operations have completed),
  // which means "chunk c has landed" only while the chunk requests - three per wave and chunk - are the wave's only
  // vector-memory operations in flight: Q is finished and the counter drained before the first request, block ids come
  // through the scalar cache, the output stores follow the final vmcnt(0).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int rq = 0, rq_slot = 0, rq_t = min(odd, t_max), rq_bi, rq_in;
  locate(rq_t, rq_bi, rq_in);
  int rq_blk = table_row[rq_bi];
  auto advance = [&]() __attribute__((always_inline)) {  // the request state moves to chunk min(rq + 1, r_last)
    if (rq < r_last) {
      ++rq;
      rq_slot = rq_slot + 1 == NBUF ? 0 : rq_slot + 1;
      const int t_new = min(rq_t + 2, t_max);
      rq_in += t_new - rq_t;
      rq_t = t_new;
      if (rq_in >= tpb) {
        rq_in -= tpb;
        ++rq_bi;
      }
      if (rq_in >= tpb) {  // tpb == 1: two blocks further
        rq_in -= tpb;
        ++rq_bi;
      }
      rq_bi = __builtin_amdgcn_readfirstlane(rq_bi);  // (wave-uniform: keep the index scalar)
      rq_blk = table_row[rq_bi];                      // in the loop: read one chunk AHEAD of its use
    }
  };
  request(rq_slot, rq_blk, rq_in);  // chunks 0, 1, 2 (saturating)
  advance();
  request(rq_slot, rq_blk, rq_in);
  advance();
  request(rq_slot, rq_blk, rq_in);
  advance();

  // ---- LDS byte offsets of this lane's operand pieces inside a tile
  const int k_off = hi * 256 + (n & 15) * 16;                  // K: key n = token n % 16 of tile n / 16; + i * 1024 + b * 512
  const int v_off = (hi * 16 + (n & 15)) * 16 + (n >> 4) * 4;  // V: dim 32 db + n; + (db / 2) * 1024 + (db % 2) * 8 (+ 512)
  const int s_off = KV8_DATA + 16 * hi;                        // scales of tokens 4 hi .. + 3 (+ 32: 8 + 4 hi .. + 3)

  auto attend = [&](int c, int buf) __attribute__((always_inline)) {
    if (c < wave_chunks) {
      const uint8_t* kt = &stage[buf][n >> 4][k_off];
      f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const u32x4 a = *reinterpret_cast<const u32x4*>(kt + i * 1024 + b * 512);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dq8(a[0], a[1]), Q[4 * i + b], s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dq8(a[2], a[3]), Q[4 * i + 2 + b], s, 0, 0, 0);
        }
      // register i of this lane: key c * 32 + (i & 3) + 8 (i >> 2) + 4 hi = token (i & 3) + 8 ((i >> 2) & 1) + 4 hi of
      // tile i >> 3; its scales are components i & 3 of the 16 bytes at s_off + 32 ((i >> 2) & 1)
      float ksl[16], vsc[16];
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) {
        const f32x4 ks = *reinterpret_cast<const f32x4*>(&stage[buf][t4 >> 1][s_off + 32 * (t4 & 1)]);
        const f32x4 vs = *reinterpret_cast<const f32x4*>(&stage[buf][2 + (t4 >> 1)][s_off + 32 * (t4 & 1)]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ksl[4 * t4 + r] = ks[r] * scale_log2e;
          vsc[4 * t4 + r] = vs[r];
        }
      }
      const int tok0 = c * 32 + 4 * hi;
      if (c * 32 + 32 > limit_all) {  // wave-uniform: some column does not see the whole chunk
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (tok0 + (i & 3) + 8 * (i >> 2) >= limit) {  // (whatever the slot holds: the score is -inf, its scale sane)
            s[i] = -INFINITY;
            ksl[i] = scale_log2e;
            vsc[i] = 0.f;
          }
      }
      float p[16];
      auto chunk_max = [&]() __attribute__((always_inline)) {
        float t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = s[i] * ksl[i];
        float mc = fmaxf(fmaxf(fmaxf(fmaxf(t[0], t[1]), t[2]), fmaxf(fmaxf(t[3], t[4]), t[5])),
                         fmaxf(fmaxf(fmaxf(t[6], t[7]), t[8]), fmaxf(fmaxf(t[9], t[10]), t[11])));
        mc = fmaxf(mc, fmaxf(fmaxf(fmaxf(t[12], t[13]), t[14]), t[15]));
        return xor32_max(mc);
      };
      auto rescale_to = [&](float mn) __attribute__((always_inline)) {
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        l *= alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[j][i] *= alpha;
        m = mn;
      };
      auto exps = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], ksl[i], -m));
        return ((p[0] + p[4]) + (p[8] + p[12])) + ((p[1] + p[5]) + (p[9] + p[13])) +
               (((p[2] + p[6]) + (p[10] + p[14])) + ((p[3] + p[7]) + (p[11] + p[15])));
      };
      // the bf16 kernel's test: a lane's sixteen exponentials against the current reference point add up to at most
      // 2^kDeferMax exactly when none of them is larger; m = -inf at the first chunk gives inf or NaN, the comparison
      // fails and the slow path sets the reference point (finite from chunk 0 on: key 0 is visible to every column)
      float lc = exps();
      if (__any(!(lc <= 256.0f))) {
        rescale_to(fmaxf(m, chunk_max()));
        lc = exps();
      }
      l += lc;  // the sum is over the probabilities; V's scale belongs to the numerator only
      u32x4 ph[2];
#pragma unroll
      for (int i = 0; i < 8; ++i) ph[i >> 2][i & 3] = pack_bf(p[2 * i] * vsc[2 * i], p[2 * i + 1] * vsc[2 * i + 1]);
#pragma unroll
      for (int sgm = 0; sgm < 2; ++sgm) {
        const uint8_t* vt = &stage[buf][2 + sgm][v_off];
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const uint32_t w0 = *reinterpret_cast<const uint32_t*>(vt + (db >> 1) * 1024 + (db & 1) * 8);
          const uint32_t w1 = *reinterpret_cast<const uint32_t*>(vt + (db >> 1) * 1024 + (db & 1) * 8 + 512);
          acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dq8(w0, w1), as_frag(ph[sgm]), acc[db], 0, 0, 0);
        }
      }
    }
  };
  int rd_slot = 0;
  for (int c = 0; c < wg_chunks; ++c) {
    // this wave's pieces of chunk c have landed (those of c + 1 and c + 2 may still fly); after the barrier everybody's
    // have, and everybody is done reading chunk c - 1, whose slot chunk c + 3 re-uses
    asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
    request(rq_slot, rq_blk, rq_in);
    advance();
    attend(c, rd_slot);
    rd_slot = rd_slot + 1 == NBUF ? 0 : rd_slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the padding requests
  __syncthreads();
  l = xor32_sum(l);
  // O^T -> rows through the idle stage, as the bf16 kernel: each wave transposes its [128 dims][32 cols] tile through
  // its own 8 KiB, column n's 256-byte row XOR-swizzled in 8-byte pieces
  uint16_t* tile = reinterpret_cast<uint16_t*>(&stage[0][0][0]) + wave * (32 * D);
  const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      const int piece8 = db * 8 + i4 * 2 + hi;  // dims 4 piece8 .. + 3  (= 32 db + 8 i4 + 4 hi)
      u32x2 o;
      o[0] = pack_bf(acc[db][4 * i4] * inv, acc[db][4 * i4 + 1] * inv);
      o[1] = pack_bf(acc[db][4 * i4 + 2] * inv, acc[db][4 * i4 + 3] * inv);
      *reinterpret_cast<u32x2*>(tile + n * D + ((piece8 ^ n) & 31) * 4) = o;
    }
  // same wave wrote and reads: LDS operations of a wave complete in order
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int col = it * 4 + lane / 16, dl = lane % 16;
    const int qt = qt0 + col / G;
    const u32x2 lo = *reinterpret_cast<const u32x2*>(tile + col * D + (((2 * dl) ^ col) & 31) * 4);
    const u32x2 hh = *reinterpret_cast<const u32x2*>(tile + col * D + (((2 * dl + 1) ^ col) & 31) * 4);
    if (wave_on && qt < q_len) {
      uint16_t* op = out + ((int64_t)(q_start + qt) * n_q_heads + h * G + col % G) * D + 8 * dl;
      *reinterpret_cast<u32x4*>(op) = u32x4{lo[0], lo[1], hh[0], hh[1]};
    }
  }
}

// ---------------------------------------------------------------------------
// The K / V front of a prefill step in one launch: k-norm + RoPE on K and the quantising store of K and V, from the
// packed qkv rows.  One workgroup per (16 consecutive tokens, kv head), 16 groups of 8 lanes with one token each: the
// arithmetic of mi_rmsnorm -> mi_rope (head_rmsnorm / head_rope, kv_store.hpp) and the expressions of
// kv_store_fp8_kernel, so every byte and scale is the launch sequence's.  Both tiles are assembled in LDS as stored;
// when the 16 slots fill one aligned tile (always, for a sequence that starts on a block boundary) they leave as two
// coalesced runs of 2112 bytes, otherwise every live token scatters its own bytes (negative slots are skipped).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(128) void qknorm_rope_store_fp8_kernel(
    const uint16_t* __restrict__ qkv, int64_t row_stride, const uint16_t* __restrict__ k_w, float eps,
    const int64_t* __restrict__ positions, const float* __restrict__ cos_sin, uint8_t* __restrict__ k_cache,
    uint8_t* __restrict__ v_cache, const int32_t* __restrict__ slots, int n_tokens, int n_q_heads, int n_kv_heads,
    int block_size) {
  __shared__ __attribute__((aligned(16))) uint8_t img[2][KV8_TILE];  // the K and the V tile as stored
  __shared__ int sm_slot[16];
  const int t0 = blockIdx.x * 16, h = blockIdx.y, tid = threadIdx.x;
  const int tk = tid >> 3, j = tid & 7;
  const int n_here = min(16, n_tokens - t0);
  const bool live = tk < n_here;
  const int token = live ? t0 + tk : t0;  // idle groups shadow a valid token (the reductions stay defined)
  if (tid < 16) sm_slot[tid] = tid < n_here ? slots[t0 + tid] : -2;
  const uint16_t* row = qkv + (int64_t)token * row_stride;
  uint32_t q4[2][4];  // [K | V][dims 8 j .. + 3, + 4 .., 64 + 8 j .., 64 + 8 j + 4 ..]
  float scale[2];
#pragma unroll
  for (int is_v = 0; is_v < 2; ++is_v) {
    const uint16_t* src = row + (int64_t)(n_q_heads + is_v * n_kv_heads + h) * 128;
    float a[8], b[8];
    load16(src + 8 * j, a);
    load16(src + 64 + 8 * j, b);
    if (!is_v) {
      if (k_w != nullptr) head_rmsnorm(a, b, k_w, j, eps);
      head_rope(a, b, cos_sin + positions[token] * 128, j);
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fmaxf(fabsf(a[i]), fabsf(b[i])));
    amax = xor_max<1>(amax);
    amax = xor_max<2>(amax);
    amax = xor_max<4>(amax);
    const int e = kv8_exponent(amax);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
    scale[is_v] = __uint_as_float((uint32_t)(127 + e) << 23);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      q4[is_v][i] = quant4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], inv);
      q4[is_v][2 + i] = quant4(b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3], inv);
    }
  }
  // one token's bytes into a K tile / a V tile at `kt` / `vt` (LDS image or the cache itself)
  auto put = [&](uint8_t* kt, uint8_t* vt, int t) __attribute__((always_inline)) {
    *reinterpret_cast<u32x2*>(kt + k8_tile_off(t, 8 * j)) = u32x2{q4[0][0], q4[0][1]};
    *reinterpret_cast<u32x2*>(kt + k8_tile_off(t, 64 + 8 * j)) = u32x2{q4[0][2], q4[0][3]};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      vt[v8_tile_off(t, 8 * j + i)] = (uint8_t)(q4[1][i >> 2] >> (8 * (i & 3)));
      vt[v8_tile_off(t, 64 + 8 * j + i)] = (uint8_t)(q4[1][2 + (i >> 2)] >> (8 * (i & 3)));
    }
    if (j == 0) {
      *reinterpret_cast<float*>(kt + KV8_DATA + 4 * t) = scale[0];
      *reinterpret_cast<float*>(vt + KV8_DATA + 4 * t) = scale[1];
    }
  };
  put(img[0], img[1], tk);
  __syncthreads();
  const int s0 = sm_slot[0];
  bool tile_ok = s0 >= 0 && (s0 & 15) == 0;
#pragma unroll
  for (int i = 1; i < 16; ++i) tile_ok = tile_ok && sm_slot[i] == s0 + i;
  const int tpb = block_size >> 4;
  if (tile_ok) {  // 132 pieces of 16 bytes per tile
    const int64_t base = kv8_tile_base(s0 / block_size, h, s0 % block_size, n_kv_heads, tpb);
    for (int oc = tid; oc < KV8_TILE / 16; oc += 128) {
      *reinterpret_cast<u32x4*>(k_cache + base + oc * 16) = *reinterpret_cast<const u32x4*>(&img[0][oc * 16]);
      *reinterpret_cast<u32x4*>(v_cache + base + oc * 16) = *reinterpret_cast<const u32x4*>(&img[1][oc * 16]);
    }
  } else if (live) {
    const int sl = sm_slot[tk];
    if (sl >= 0) {
      const int64_t base = kv8_tile_base(sl / block_size, h, sl % block_size, n_kv_heads, tpb);
      put(k_cache + base, v_cache + base, sl & 15);
    }
  }
}

static int prefill8_impl(const mi_bf16* q, int64_t q_row_stride, const QPrep* prep, const uint8_t* k_cache,
                         const uint8_t* v_cache, const int32_t* block_table, int table_stride,
                         const int32_t* cu_seqlens_q, const int32_t* kv_lens, int n_seqs, int max_seqlen_q, mi_bf16* out,
                         int n_q_heads, int n_kv_heads, int head_dim, int block_size, float scale, mi_stream stream) {
  if (!q || !k_cache || !v_cache || !block_table || !cu_seqlens_q || !kv_lens || !out) return MI_EINVAL;
  if (n_q_heads <= 0 || n_seqs < 0 || max_seqlen_q < 0 || table_stride <= 0) return MI_EINVAL;
  int rc = check_kv8(n_kv_heads, head_dim, block_size);
  if (rc != MI_OK) return rc;
  if (q_row_stride % 8 || n_q_heads % n_kv_heads) return MI_EUNSUPPORTED;
  const int G = n_q_heads / n_kv_heads;
  if (G != 1 && G != 2 && G != 4 && G != 8 && G != 16) return MI_EUNSUPPORTED;
  if (!aligned16(q) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(out)) return MI_EINVAL;
  if (n_seqs == 0 || max_seqlen_q == 0) return MI_OK;
  if ((int64_t)n_kv_heads * (block_size / 16) * KV8_TILE > INT32_MAX) return MI_EUNSUPPORTED;  // 32-bit block stride
  const int tq_wg = 4 * (32 / G);  // query tokens per workgroup
  const int n_qblocks = (max_seqlen_q + tq_wg - 1) / tq_wg;
  const int64_t n_pairs = (int64_t)n_seqs * n_kv_heads, n_wg = (n_pairs + 7) / 8 * 8 * n_qblocks;
  if (n_wg > INT32_MAX) return MI_EUNSUPPORTED;
  const dim3 grid((unsigned)n_wg);
  const float sl2 = scale * 1.4426950408889634f;
  int tpb_shift = -1;  // log2 of the tiles per block, or -1 (division) for block sizes like 48
  for (int sft = 0; sft < 12; ++sft)
    if ((1 << sft) == block_size / 16) tpb_shift = sft;
  hipStream_t st = S(stream);
  const QPrep qp = prep ? *prep : QPrep{nullptr, nullptr, nullptr, 0.f};
#define LAUNCH_PRE8_AS(GG, FQ)                                                                                          \
  hipLaunchKernelGGL((paged_attn_prefill_fp8kv_kernel<GG, FQ>), grid, dim3(256), 0, st, q, q_row_stride, k_cache, v_cache, \
                     block_table, table_stride, cu_seqlens_q, kv_lens, out, n_q_heads, n_kv_heads, block_size / 16,     \
                     tpb_shift, sl2, n_qblocks, (int)n_pairs, qp)
#define LAUNCH_PRE8(GG)                 \
  if (prep) LAUNCH_PRE8_AS(GG, true);   \
  else LAUNCH_PRE8_AS(GG, false)
  switch (G) {
    case 1: LAUNCH_PRE8(1); break;
    case 2: LAUNCH_PRE8(2); break;
    case 4: LAUNCH_PRE8(4); break;
    case 8: LAUNCH_PRE8(8); break;
    default: LAUNCH_PRE8(16); break;
  }
#undef LAUNCH_PRE8
#undef LAUNCH_PRE8_AS
  return check_launch();
}

}  // namespace mi

using namespace mi;

// attention.py:37-62 (the prefill branch) over the fp8 cache
extern "C" int mi_paged_attn_prefill_fp8kv(const mi_bf16* q, int64_t q_row_stride, const uint8_t* k_cache,
                                           const uint8_t* v_cache, const int32_t* block_table, int table_stride,
                                           const int32_t* cu_seqlens_q, const int32_t* kv_lens, int n_seqs,
                                           int max_seqlen_q, mi_bf16* out, int n_q_heads, int n_kv_heads, int head_dim,
                                           int block_size, float scale, mi_stream stream) {
  return prefill8_impl(q, q_row_stride, nullptr, k_cache, v_cache, block_table, table_stride, cu_seqlens_q, kv_lens, n_seqs,
                       max_seqlen_q, out, n_q_heads, n_kv_heads, head_dim, block_size, scale, stream);
}

// qwen3.py:83-88 (the query side) + attention.py:37-62 over the fp8 cache, straight from the packed qkv rows
extern "C" int mi_paged_attn_prefill_fp8kv_fused(const mi_bf16* qkv, int64_t qkv_row_stride, const mi_bf16* q_w, float eps,
                                                 const int64_t* positions, const float* cos_sin, const uint8_t* k_cache,
                                                 const uint8_t* v_cache, const int32_t* block_table, int table_stride,
                                                 const int32_t* cu_seqlens_q, const int32_t* kv_lens, int n_seqs,
                                                 int max_seqlen_q, mi_bf16* out, int n_q_heads, int n_kv_heads,
                                                 int head_dim, int block_size, float scale, mi_stream stream) {
  if (!positions || !cos_sin || !aligned16(cos_sin) || (q_w && !aligned16(q_w))) return MI_EINVAL;
  const QPrep prep{q_w, positions, cos_sin, eps};
  return prefill8_impl(qkv, qkv_row_stride, &prep, k_cache, v_cache, block_table, table_stride, cu_seqlens_q, kv_lens,
                       n_seqs, max_seqlen_q, out, n_q_heads, n_kv_heads, head_dim, block_size, scale, stream);
}

// qwen3.py:83-88 (the key side) + attention.py:22-35 over the fp8 cache: mi_rmsnorm (k), mi_rope and mi_kv_store_fp8 in one
extern "C" int mi_qknorm_rope_store_fp8(const mi_bf16* qkv, int64_t qkv_row_stride, const mi_bf16* k_w, float eps,
                                        const int64_t* positions, const float* cos_sin, uint8_t* k_cache,
                                        uint8_t* v_cache, const int32_t* slot_flat, int n_tokens, int n_q_heads,
                                        int n_kv_heads, int head_dim, int block_size, mi_stream stream) {
  if (!qkv || !positions || !cos_sin || !k_cache || !v_cache || !slot_flat || n_tokens < 0 || n_q_heads <= 0)
    return MI_EINVAL;
  int rc = check_kv8(n_kv_heads, head_dim, block_size);
  if (rc != MI_OK) return rc;
  if (qkv_row_stride % 8) return MI_EUNSUPPORTED;
  if (!aligned16(qkv) || !aligned16(k_cache) || !aligned16(v_cache) || !aligned16(cos_sin) || (k_w && !aligned16(k_w)))
    return MI_EINVAL;
  if (n_tokens == 0) return MI_OK;
  if (n_kv_heads > 65535) return MI_EUNSUPPORTED;
  hipLaunchKernelGGL(qknorm_rope_store_fp8_kernel, dim3((n_tokens + 15) / 16, n_kv_heads), dim3(128), 0, S(stream), qkv,
                     qkv_row_stride, k_w, eps, positions, cos_sin, k_cache, v_cache, slot_flat, n_tokens, n_q_heads,
                     n_kv_heads, block_size);
  return check_launch();
}
