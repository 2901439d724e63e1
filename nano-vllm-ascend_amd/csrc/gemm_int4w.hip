// int4 (group-128) weight-only GEMMs for the decode regime: entry points and launch selection.
// The kernel and the format are described in gemm_int4w_kernel.hpp.
#include "gemm_int4w_kernel.hpp"

using namespace mi;

namespace {

struct Int4Args {
  const uint16_t* x;
  const uint8_t* w;
  const uint16_t* sc;
  uint16_t* y;
  float* part;
  int M, N, K, ksplit;
  hipStream_t st;
};

// Waves per workgroup the register file allows.  The double-buffered loop keeps two sets of {RT weight fragments, RT
// scales, 16 MT registers of x lines} besides the B fragments and the accumulators: a 16-wave workgroup (128 VGPRs per
// lane) holds that for 16 activation rows, a 12-wave one (168) for 32 rows with one row tile; 64 rows with two row tiles
// need the whole file (4 waves); everything else runs at most 8 waves (256 VGPRs).  A wave with a single group (ONE) has
// one set: 16 waves up to 32 rows.  Checked against the compiler's resource report: no instantiation uses scratch.
constexpr int int4_max_waves(int MT, int RT, bool ONE) {
  if (ONE) return MT <= 2 ? 16 : 8;
  if (MT == 1) return 16;
  if (MT == 2 && RT == 1) return 12;
  return MT == 4 && RT == 2 ? 4 : 8;
}

template <int MT, int RT, int WAVES, int EPI, bool ONE>
void launch_int4(const Int4Args& a) {
  const size_t slot = (size_t)RT * MT * 1024 > (size_t)x_slab_bytes(MT) ? (size_t)RT * MT * 1024 : (size_t)x_slab_bytes(MT);
  const int tiles = a.N / 16, kslice = a.K / (a.ksplit * WAVES);
  const dim3 grid(EPI == EPI_SILU ? tiles / 2 : tiles / RT, a.ksplit, (a.M + kSkinnyRows - 1) / kSkinnyRows);
  hipLaunchKernelGGL((gemm_int4w_kernel<MT, RT, WAVES, EPI, ONE>), grid, dim3(WAVES * 64), WAVES * slot, a.st, a.x, a.w,
                     a.sc, a.M, a.N, a.K, kslice, a.y, a.part);
}

template <int MT, int RT, int WAVES, int EPI, bool ONE>
bool try_int4_form(const Int4Args& a) {
  if constexpr (WAVES > int4_max_waves(MT, RT, ONE)) {
    return false;
  } else {
    launch_int4<MT, RT, WAVES, EPI, ONE>(a);
    return true;
  }
}

template <int MT, int RT, int WAVES, int EPI>
bool try_int4(const Int4Args& a, int groups, int cap) {
  if (WAVES > cap || groups % WAVES) return false;
  return groups == WAVES ? try_int4_form<MT, RT, WAVES, EPI, true>(a) : try_int4_form<MT, RT, WAVES, EPI, false>(a);
}

// As pick_waves of the bf16 kernels, in units of one group (128 k): one group per wave while that fits the workgroup -
// these launches are latency-bound, so the fewer dependent loads a wave issues the better - else the most waves that
// divide the groups; many row tiles (>= 2048 workgroups): at most four, fatter, waves.
template <int MT, int RT, int EPI>
int pick_int4_waves(const Int4Args& a) {
  const int groups = a.K / (128 * a.ksplit);
  const int wgs = (a.N / 16) / (EPI == EPI_SILU ? 2 : RT) * a.ksplit;
  const int cap = wgs >= 2048 ? 4 : 16;
  const bool ok = try_int4<MT, RT, 16, EPI>(a, groups, cap) || try_int4<MT, RT, 12, EPI>(a, groups, cap) ||
                  try_int4<MT, RT, 8, EPI>(a, groups, cap) || try_int4<MT, RT, 7, EPI>(a, groups, cap) ||
                  try_int4<MT, RT, 4, EPI>(a, groups, cap) || try_int4<MT, RT, 2, EPI>(a, groups, cap) ||
                  try_int4<MT, RT, 1, EPI>(a, groups, cap);
  return ok ? check_launch() : MI_EUNSUPPORTED;
}

template <int RT, int EPI>
int pick_int4_mt(const Int4Args& a) {
  switch ((min(a.M, kSkinnyRows) + 15) / 16) {
    case 1: return pick_int4_waves<1, RT, EPI>(a);
    case 2: return pick_int4_waves<2, RT, EPI>(a);
    case 3: return pick_int4_waves<3, RT, EPI>(a);
    default: return pick_int4_waves<4, RT, EPI>(a);
  }
}

// the checks of every int4 GEMM entry point, all on the host and in front of any launch
int check_int4(const void* x, const void* w, const void* scale, const void* out, int M, int N, int K) {
  const int rc = check_gemm(x, w, out, M, N, K);
  if (rc != MI_OK) return rc;
  if (!scale || !aligned16(scale)) return MI_EINVAL;
  if (K % 128) return MI_EUNSUPPORTED;
  return MI_OK;
}

}  // namespace

extern "C" int mi_pack_weight_int4(const uint8_t* q, const mi_bf16* scale, uint8_t* w_packed, mi_bf16* scale_packed,
                                   int N, int K, mi_stream stream) {
  if (!q || !scale || !w_packed || !scale_packed || N <= 0 || K <= 0) return MI_EINVAL;
  if (N % 16 || K % 128) return MI_EUNSUPPORTED;
  if (!aligned16(q) || !aligned16(w_packed) || !aligned16(scale_packed)) return MI_EINVAL;
  const int64_t chunks = (int64_t)N * K / 32;
  hipLaunchKernelGGL(pack_weight_int4_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, S(stream), q, scale,
                     w_packed, scale_packed, N, K);
  return check_launch();
}

extern "C" int mi_gemm_int4w_packed(const mi_bf16* x, const uint8_t* w_packed, const mi_bf16* scale_packed, mi_bf16* y,
                                    int M, int N, int K, int epilogue, mi_stream stream) {
  const int rc = check_int4(x, w_packed, scale_packed, y, M, N, K);
  if (rc != MI_OK) return rc;
  if (epilogue != 0 && epilogue != 1) return MI_EINVAL;
  if (epilogue == 1 && N % 32) return MI_EUNSUPPORTED;
  if (M == 0) return MI_OK;
  const Int4Args a{x, w_packed, scale_packed, y, nullptr, M, N, K, 1, S(stream)};
  if (epilogue == 1) return pick_int4_mt<2, EPI_SILU>(a);
  // two row tiles per workgroup halve the x traffic per weight byte once there are plenty of tiles
  if (N / 16 >= 1024 && (N / 16) % 2 == 0 && M <= 32) return pick_int4_mt<2, EPI_NONE>(a);
  return pick_int4_mt<1, EPI_NONE>(a);
}

extern "C" int mi_gemm_int4w_packed_splitk(const mi_bf16* x, const uint8_t* w_packed, const mi_bf16* scale_packed,
                                           float* partials, int M, int N, int K, int ksplit, mi_stream stream) {
  const int rc = check_int4(x, w_packed, scale_packed, partials, M, N, K);
  if (rc != MI_OK) return rc;
  if (ksplit < 1 || ksplit > 16 || K % (128 * ksplit)) return MI_EUNSUPPORTED;
  if (M == 0) return MI_OK;
  return pick_int4_mt<1, EPI_PARTIAL>(Int4Args{x, w_packed, scale_packed, nullptr, partials, M, N, K, ksplit, S(stream)});
}
