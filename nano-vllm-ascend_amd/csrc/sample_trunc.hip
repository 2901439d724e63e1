// Top-k / top-p (nucleus) sampling over [rows][vocab] bf16 logits: mi_sample_truncated (include/mi355_nanovllm.h).
//
// The sampler of this library is Gumbel-max (mi_common.hpp: token = argmax_c gumbel_key(logit_c, 1/T, rkey, c)), so
// truncated sampling is the same arg-max over the KEPT columns.  One 1024-lane workgroup per row finds the kept set
// as a threshold on the bf16 VALUE and takes the arg-max above it with the keys of mi_sample:
//
//   * a bf16 has 16 bits: bf_key() maps the pattern to an unsigned 16-bit key that orders as the float does (+0 and -0
//     share a key), so "the k-th largest value" and "the smallest value set of mass >= p" are both radix selects over
//     65536 values in two 8-bit levels, and the kept set is `key >= threshold`;
//   * the row is loaded ONCE, with 16-byte loads, into registers (19 x 4 packed dwords per lane hold 155648 columns:
//     Qwen3's 151936 and Llama's 128256) and every pass - maximum, two count levels, two mass levels, the arg-max -
//     runs from there; longer rows take the same passes over memory (L2-resident after the first);
//   * the hi byte of a bf16 is sign + 7 exponent bits, so a level-1 histogram of real logits has a handful of hot bins:
//     LDS bins are laid out [bin][copy] with copy = lane % COPIES, which puts the lanes of a half-wave on different
//     banks whatever bins they hit (no same-address serialisation); the copies are summed afterwards;
//   * the top-p mass is summed as 64-bit fixed point (exp((l - max)/T) * 2^40, integer LDS adds): the sum does not
//     depend on the order in which lanes arrive, so equal inputs give equal tokens on every run;
//   * after truncation the kept columns are few: the Gumbel keys (two logf and a 64-bit mix per column - what bounds
//     mi_sample) are formed only where a wave holds a kept column.
#include "mi_common.hpp"

namespace mi {

constexpr int ST_THREADS = 1024;
constexpr int ST_BIN_BYTES = 32 * 1024;  // [256 bins][copies] of uint32 counts (32 copies) or uint64 masses (16)
constexpr float ST_MASS_ONE = 1099511627776.0f;  // 2^40: weights are <= 1, a row of 2^17 columns sums below 2^58

// bf16 bit pattern -> unsigned 16-bit key, monotone in the float value; -0.0 gets the key of +0.0
__device__ __forceinline__ uint32_t bf_key(uint32_t h) {
  h = h == 0x8000u ? 0u : h;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
__device__ __forceinline__ float key_value(uint32_t key) {
  return bf2f((uint16_t)((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu)));
}

// The row of one workgroup.  NV > 0: vectors v = lane + i * 1024 (i < NV) live in registers (every loop over them is
// unrolled: the array never leaves the register file); NV == 0: every pass reads memory.  Columns behind the last
// whole vector (vocab % 8) are read as scalars by the first lanes, as scan_row (elementwise.hip) does.
template <int NV>
struct Row {
  u32x4 r[NV > 0 ? NV : 1];
  const uint16_t* p;
  int vocab, nvec;

  __device__ __forceinline__ void load(const uint16_t* row, int vocab_) {
    p = row;
    vocab = vocab_;
    nvec = vocab_ >> 3;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * ST_THREADS;
      r[i] = u32x4{0, 0, 0, 0};
      if (v < nvec) r[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + (int64_t)v * 8));
    }
  }
  // f(raw, v) for every whole vector of this lane
  template <class F>
  __device__ __forceinline__ void vectors(F&& f) const {
    if constexpr (NV > 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int v = threadIdx.x + i * ST_THREADS;
        if (v < nvec) f(r[i], v);
      }
    } else {
      for (int v = threadIdx.x; v < nvec; v += ST_THREADS) f(*reinterpret_cast<const u32x4*>(p + (int64_t)v * 8), v);
    }
  }
  template <class F>
  __device__ __forceinline__ void tail(F&& f) const {  // f(bits, col)
    for (int col = (nvec << 3) + threadIdx.x; col < vocab; col += ST_THREADS) f((uint32_t)p[col], col);
  }
  // f(bits, col) for every column of this lane
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
    vectors([&](const u32x4& raw, int v) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(raw[j] & 0xffffu, v * 8 + 2 * j);
        f(raw[j] >> 16, v * 8 + 2 * j + 1);
      }
    });
    tail(f);
  }
};

struct SelectScratch {
  uint64_t tot[256];   // per-bin totals of the level at hand
  uint64_t above;      // what lies strictly above the selected bin (counts or mass)
  uint64_t total;      // everything in the level's bins plus what was above them
  int bin;
  int wave_max[16];
};

__device__ __forceinline__ void zero_bins(uint32_t* bins) {
  u32x4* b = reinterpret_cast<u32x4*>(bins);
#pragma unroll
  for (int i = 0; i < ST_BIN_BYTES / 16 / ST_THREADS; ++i) b[threadIdx.x + i * ST_THREADS] = u32x4{0, 0, 0, 0};
  __syncthreads();
}

template <class T>
__device__ __forceinline__ void bin_add(uint32_t* bins, uint32_t bin, T val) {
  constexpr int COPIES = ST_BIN_BYTES / 256 / (int)sizeof(T);
  atomicAdd(reinterpret_cast<T*>(bins) + bin * COPIES + (threadIdx.x & (COPIES - 1)), val);
}

// the smallest integer mass >= share * total, at least one unit (a share of 0 keeps the row maximum)
__device__ __forceinline__ uint64_t share_of(float share, uint64_t total) {
  const double want = (double)fmaxf(share, 0.f) * (double)total;
  uint64_t target = (uint64_t)want;
  if ((double)target < want) ++target;
  return target ? target : 1;
}

// The bins of one level are full (the caller has not synchronised yet).  Selects the LARGEST bin b with
// above + sum(bins >= b) >= target and leaves {bin, what lies above it, the level's total + above} in s; bin 0 if
// there is none.  All 1024 lanes call it; the result is readable by all of them on return.
template <class T>
__device__ __forceinline__ void select_bin(const uint32_t* bins, SelectScratch& s, uint64_t above, uint64_t target,
                                           bool target_is_share, float share) {
  constexpr int COPIES = ST_BIN_BYTES / 256 / (int)sizeof(T);
  constexpr int PER = COPIES / 4;  // four lanes per bin
  __syncthreads();
  {
    const T* b = reinterpret_cast<const T*>(bins) + (threadIdx.x >> 2) * COPIES + (threadIdx.x & 3) * PER;
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) sum += b[i];
    sum += __shfl_xor((unsigned long long)sum, 1, 64);
    sum += __shfl_xor((unsigned long long)sum, 2, 64);
    if ((threadIdx.x & 3) == 0) s.tot[threadIdx.x >> 2] = sum;
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // lane L owns bins 4 L .. 4 L + 3; suffix sums over the lanes, then inside the lane
    const int lane = threadIdx.x;
    uint64_t a[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = s.tot[lane * 4 + j];
      mine += a[j];
    }
    uint64_t suffix = mine;  // sum over lanes >= lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t up = __shfl_down((unsigned long long)suffix, o, 64);
      if (lane + o < 64) suffix += up;
    }
    const uint64_t total = above + __shfl((unsigned long long)suffix, 0, 64);
    if (target_is_share) target = share_of(share, total);
    uint64_t run = above + suffix - mine;  // everything above this lane's bins
    int found = -1;
    uint64_t found_above = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const uint64_t before = run;
      run += a[j];
      if (found < 0 && run >= target) {
        found = lane * 4 + j;
        found_above = before;
      }
    }
    const uint64_t who = __ballot(found >= 0);
    if (who == 0) {
      if (lane == 0) {
        s.bin = 0;
        s.above = total - a[0];
        s.total = total;
      }
    } else if (lane == 63 - __builtin_clzll(who)) {
      s.bin = found;
      s.above = found_above;
      s.total = total;
    }
  }
  __syncthreads();
}

// Two-level radix select.  weight(bits) is the contribution of a column (1 for counts, the fixed-point mass for
// top-p), taken over the columns with key >= floor_key.  Returns the largest key t with sum(weight of key >= t) >=
// target (target_is_share: >= share * the sum over all of them).
template <class T, int NV, class W>
__device__ __forceinline__ uint32_t radix_select(const Row<NV>& row, uint32_t* bins, SelectScratch& s, uint32_t floor_key,
                                                 uint64_t target, bool target_is_share, float share, W&& weight) {
  zero_bins(bins);
  row.each([&](uint32_t h, int) {
    const uint32_t key = bf_key(h);
    if (key >= floor_key) bin_add<T>(bins, key >> 8, (T)weight(h));
  });
  select_bin<T>(bins, s, 0, target, target_is_share, share);
  const uint32_t hi = (uint32_t)s.bin;
  const uint64_t above = s.above;
  if (target_is_share) target = share_of(share, s.total);  // the second level compares with the same absolute mass
  zero_bins(bins);  // (its barrier also orders the reads of s above before select_bin writes it again)
  row.each([&](uint32_t h, int) {
    const uint32_t key = bf_key(h);
    if (key >= floor_key && (key >> 8) == hi) bin_add<T>(bins, key & 0xffu, (T)weight(h));
  });
  select_bin<T>(bins, s, above, target, false, 0.f);
  return (hi << 8) | (uint32_t)s.bin;
}

template <int NV>
__global__ __launch_bounds__(ST_THREADS) void sample_truncated_kernel(
    const uint16_t* __restrict__ logits, int64_t row_stride, const float* __restrict__ temperatures,
    const int32_t* __restrict__ top_k, const float* __restrict__ top_p, int64_t* __restrict__ out, int vocab,
    uint64_t seed, uint64_t step, const uint64_t* __restrict__ rng) {
  const int row = blockIdx.x;
  const int k = top_k[row];
  const float share = top_p[row];
  if (k <= 0 && !(share < 1.0f)) return;  // truncation off: the row keeps the token the step's own pick wrote
  __shared__ __attribute__((aligned(16))) uint32_t bins[ST_BIN_BYTES / 4];
  __shared__ SelectScratch s;
  __shared__ float sb[16];
  __shared__ int si[16];
  if (rng) {
    seed = rng[0];
    step = rng[1];
  }
  const float t = temperatures[row];
  const bool noisy = t > 0.f;
  const float inv_t = noisy ? 1.0f / t : 1.0f;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  Row<NV> data;
  data.load(logits + (int64_t)row * row_stride, vocab);

  uint32_t keep = 0;  // the kept set: bf_key >= keep
  if (noisy) {        // (a greedy row takes the arg-max, which every truncation keeps)
    if (k > 0 && k < vocab)
      keep = radix_select<uint32_t>(data, bins, s, 0u, (uint64_t)k, false, 0.f, [](uint32_t) { return 1u; });
    if (share < 1.0f) {
      int top = 0;  // the row maximum, as a key
      data.each([&](uint32_t h, int) { top = max(top, (int)bf_key(h)); });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
      if (lane == 0) s.wave_max[wave] = top;
      __syncthreads();
#pragma unroll
      for (int wv = 0; wv < ST_THREADS / 64; ++wv) top = max(top, s.wave_max[wv]);
      const float row_max = key_value((uint32_t)top);
      if (row_max > -INFINITY) {  // (a row of -inf has no mass to share out: top-k alone decides)
        keep = radix_select<uint64_t>(data, bins, s, keep, 0, true, share, [&](uint32_t h) {
          const float l = bf2f((uint16_t)h);
          return l == -INFINITY ? 0ull : (uint64_t)(__expf((l - row_max) * inv_t) * ST_MASS_ONE);
        });
      }
    }
  }

  // arg-max of the sampler's keys over the kept columns: value first, then the lowest column (pick_kernel)
  const uint64_t rkey = sample_row_key(seed, step, row);
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  auto consider = [&](uint32_t h, int col) {
    if (bf_key(h) < keep) return;
    float key = bf2f((uint16_t)h);
    if (noisy) key = gumbel_key(key, inv_t, rkey, col);
    if (key > best || (key == best && col < best_i)) {
      best = key;
      best_i = col;
    }
  };
  data.vectors([&](const u32x4& raw, int v) {
    // one body per vector, not per column: the column loop stays a loop (j is wave-uniform, the dword is selected)
#pragma nounroll
    for (int j = 0; j < 8; ++j) {
      const int d = j >> 1;
      const uint32_t w = d == 0 ? raw[0] : d == 1 ? raw[1] : d == 2 ? raw[2] : raw[3];
      consider((j & 1) ? (w >> 16) : (w & 0xffffu), v * 8 + j);
    }
  });
  data.tail(consider);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    if (ob > best || (ob == best && oi < best_i)) {
      best = ob;
      best_i = oi;
    }
  }
  if (lane == 0) {
    sb[wave] = best;
    si[wave] = best_i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < ST_THREADS / 64; ++wv)
      if (sb[wv] > best || (sb[wv] == best && si[wv] < best_i)) {
        best = sb[wv];
        best_i = si[wv];
      }
    out[row] = best_i == 0x7fffffff ? 0 : best_i;
  }
}

static int launch_sample_truncated(const mi_bf16* logits, int64_t row_stride, const float* temperatures,
                                   const int32_t* top_k, const float* top_p, int64_t* out, int rows, int vocab,
                                   uint64_t seed, uint64_t step, const uint64_t* rng, mi_stream stream) {
  if (!logits || !temperatures || !top_k || !top_p || !out || rows <= 0 || vocab <= 0 || row_stride < vocab)
    return MI_EINVAL;
  if (row_stride % 8 || !aligned16(logits)) return MI_EUNSUPPORTED;
  const int nvec = vocab >> 3;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(ST_THREADS), 0, S(stream), logits, row_stride, temperatures, top_k,
                       top_p, out, vocab, seed, step, rng);
    return check_launch();
  };
  if (nvec <= 4 * ST_THREADS) return go(sample_truncated_kernel<4>);
  if (nvec <= 19 * ST_THREADS) return go(sample_truncated_kernel<19>);
  return go(sample_truncated_kernel<0>);  // a row longer than the register file holds: every pass reads memory
}

}  // namespace mi

using namespace mi;

extern "C" int mi_sample_truncated(const mi_bf16* logits, int64_t row_stride, const float* temperatures,
                                   const int32_t* top_k, const float* top_p, int64_t* out, int rows, int vocab,
                                   uint64_t seed, uint64_t step, mi_stream stream) {
  return launch_sample_truncated(logits, row_stride, temperatures, top_k, top_p, out, rows, vocab, seed, step, nullptr,
                                 stream);
}

extern "C" int mi_sample_truncated_rng(const mi_bf16* logits, int64_t row_stride, const float* temperatures,
                                       const int32_t* top_k, const float* top_p, const uint64_t* rng, int64_t* out,
                                       int rows, int vocab, mi_stream stream) {
  if (!rng) return MI_EINVAL;
  return launch_sample_truncated(logits, row_stride, temperatures, top_k, top_p, out, rows, vocab, 0, 0, rng, stream);
}
