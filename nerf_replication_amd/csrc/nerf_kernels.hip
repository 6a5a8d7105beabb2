// libnerf_mi355x.so -- HIP kernels (gfx950 only) and the C ABI of include/nerf_mi355x.h.
// Build: hipcc -O3 --offload-arch=gfx950 -shared -fPIC (see csrc/Makefile).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <utility>

#include "../../include/nerf_mi355x.h"
#include "nerf_layout.h"
#include "nerf_wgrad_table.h"
#include "nerf_scan.hip.inc"
#include "nerf_mlp_f32.hip.inc"
#include "nerf_mlp_f16.hip.inc"
#include "nerf_mlp_f16s.hip.inc"
#include "nerf_mlp_f32x.hip.inc"
#include "nerf_wgrad_f32.hip.inc"
#include "nerf_mlp_bwd_f32.hip.inc"
#include "nerf_mlp_bwd_f32x.hip.inc"
#include "nerf_wgrad_bf16x3.hip.inc"
// the split-fp16 MLP kernels are compiled in a unit of their own (nerf_kernels_x.hip says why); here they are only launched
#define NERF_X_INST extern template
#include "nerf_kernels_x.inst.inc"

#include "nerf_timing_guard.h"         // after the kernel includes: refuses a build with a stray timing switch

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* what) {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return code;
}
// Every kernel launch: NERF_OK, or NERF_ERR_HIP with "<kernel>: <hip error>" in nerf_last_error().  NERF_LAUNCH names the kernel
// expression as it is written at the call (a template instance with a comma in its arguments is written, and reported, in
// parentheses).
template <class K, class... Args>
int launch(const char* name, K kernel, dim3 grid, dim3 block, hipStream_t st, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return NERF_OK;
  snprintf(g_err, sizeof(g_err), "%s: %s", name, hipGetErrorString(e));
  return NERF_ERR_HIP;
}
#define NERF_LAUNCH(kernel, grid, block, stream, ...) launch(#kernel, kernel, grid, block, stream, __VA_ARGS__)

// ------------------------------------------------------------------------------------ pack
struct PackArgs {
  const float* p[nerf::P_COUNT];
  float* out;
};

__device__ __forceinline__ float pack_weight_elem(const PackArgs& a, long long rel, int ntiles,
                                                  int which /*0 L0,1 hidden,2 L5a,3 L5b,4 feat,5 views*/,
                                                  int layer) {
  using namespace nerf;
  const int q = (int)(rel & 3);
  const int lane = (int)((rel >> 2) & 63);
  const long long blk = rel >> 8;                 // g*NT + j
  const int j = (int)(blk % ntiles);
  const int g = (int)(blk / ntiles);
  const int s = 4 * g + q, t = s >> 4, r = s & 15, h = lane >> 5;
  const int out = 32 * j + (lane & 31);
  switch (which) {
    case 0: { const int c = pe_xyz_feat(s, h); return c < 0 ? 0.f : a.p[P_W0][out * 63 + c]; }
    case 1: return a.p[2 * layer][out * 256 + act_feat(t, r, h)];
    case 2: { const int c = pe_xyz_feat(s, h); return c < 0 ? 0.f : a.p[10][out * 319 + c]; }
    case 3: return a.p[10][out * 319 + 63 + act_feat(t, r, h)];
    case 4: return a.p[P_WF][out * 256 + act_feat(t, r, h)];
    default: {
      if (t < 8) return a.p[P_WV][out * 283 + act_feat(t, r, h)];
      const int c = pe_dir_feat(r, h);
      return c < 0 ? 0.f : a.p[P_WV][out * 283 + 256 + c];
    }
  }
}

// Element `rel` of a [h][t*16 + r] block (1 << LOG2 slots per lane-half h) over the features of x in act_feat order
template <int LOG2>
__device__ __forceinline__ float act_order_value(const float* x, int rel) {
  const int h = rel >> LOG2, slot = rel & ((1 << LOG2) - 1);
  return x[nerf::act_feat(slot >> 4, slot & 15, h)];
}
// The blocks the streams share beside w_alpha (act_order_value<7>): biases [layer 0..8][h][j*16 + r], w_rgb [c][h][t*16 + r] (t < 4)
// and the head biases b_rgb[3], b_alpha.  (The weight pointer, not PackArgs, where a kernel also picks a weight matrix by a
// run-time index: a reference to the arguments there made the compiler copy them to scratch.)
__device__ __forceinline__ float pack_bias_value(const PackArgs& a, int rel) {
  const int layer = rel >> 8;
  return act_order_value<7>(layer < 8 ? a.p[2 * layer + 1] : a.p[nerf::P_BF], rel & 255);
}
__device__ __forceinline__ float pack_w_rgb_value(const float* w_rgb, int rel) {
  return act_order_value<6>(w_rgb + 128 * (rel >> 7), rel & 127);
}
__device__ __forceinline__ float pack_head_bias_value(const PackArgs& a, int rel) {
  return rel < 3 ? a.p[nerf::P_BR][rel] : a.p[nerf::P_BA][0];
}

__global__ void nerf_pack_kernel(PackArgs a) {
  using namespace nerf;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kUnfoldedFloats) return;
  constexpr long long WS = wsize(128, 8);
  float v;
  if (i < kOffL1) v = pack_weight_elem(a, i - kOffL0, 8, 0, 0);
  else if (i < kOffL5a) { const long long rel = i - kOffL1; v = pack_weight_elem(a, rel % WS, 8, 1, 1 + (int)(rel / WS)); }
  else if (i < kOffL5b) v = pack_weight_elem(a, i - kOffL5a, 8, 2, 5);
  else if (i < kOffL6) v = pack_weight_elem(a, i - kOffL5b, 8, 3, 5);
  else if (i < kOffFeat) { const long long rel = i - kOffL6; v = pack_weight_elem(a, rel % WS, 8, 1, 6 + (int)(rel / WS)); }
  else if (i < kOffViews) v = pack_weight_elem(a, i - kOffFeat, 8, 4, 0);
  else if (i < kOffBias) v = pack_weight_elem(a, i - kOffViews, 4, 5, 0);
  else if (i < kOffBiasViews) v = pack_bias_value(a, (int)(i - kOffBias));
  else if (i < kOffWAlpha) v = act_order_value<6>(a.p[P_BV], (int)(i - kOffBiasViews));      // [h][j*16 + r], j < 4
  else if (i < kOffWRgb) v = act_order_value<7>(a.p[P_WA], (int)(i - kOffWAlpha));
  else if (i < kOffHeadBias) v = pack_w_rgb_value(a.p[P_WR], (int)(i - kOffWRgb));
  else v = pack_head_bias_value(a, (int)(i - kOffHeadBias));
  a.out[i] = v;
}

// ------------------------------------------------------------------------------------ fold (nerf_layout.h kFold*)
// feature_linear folded into the views layer, from the PACKED fp32 stream, behind which nerf_pack_model writes the result (the
// fold is as fresh as the pack): Wvf = Wv[:, :256] . Wf and bvf = Wv[:, :256] . bf + bv, every element accumulated in float64
// (products of two floats are exact there) in one fixed order and rounded once to fp32.  Blocks of 256 threads = 64 outputs x 4
// quarters of the 256-term sum (partial sums meet in LDS, combined as (0 + 1) + (2 + 3)):
//   blocks 0..127    one 1-KiB block (g, j) of Wvf each: thread (lane, part) -> float4 of lane
//   blocks 128, 129  64 values of bvf each
//   blocks 130..133  copy of the views layer's direction-part blocks
//   blocks 134..136  zeros: the padding behind bvf with the ring slack, and the alignment gap in front of the region
// Element m of the inner dimension is feature act_feat(t, r, h) with  t = m >> 5, h = (m >> 2) & 1, r = (m & 3) + 4 ((m & 31) >> 3).
constexpr int kFoldBlocks = 128 + 2 + 4 + 3;
// `fold` = pk + kOffFold: what is read through pk ends at kUnfoldedFloats, what is written through fold starts there
__global__ __launch_bounds__(256) void nerf_fold_f32_kernel(const float* __restrict__ pk, float* __restrict__ fold) {
  using namespace nerf;
  __shared__ double part_sum[4][64][4];
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6, b = blockIdx.x;
  if (b >= 134) {                                   // zeros, as float4: [bvf + 128, end of the region), then [kUnfoldedFloats, kOffFold)
    constexpr int kTail4 = (int)(kFoldFloats - kFoldOffBias - 128) / 4, kGap4 = (int)(kOffFold - kUnfoldedFloats) / 4;
    static_assert(kUnfoldedFloats % 4 == 0 && kOffFold % 4 == 0 && kFoldFloats % 4 == 0 && kTail4 + kGap4 <= 3 * 256, "zero blocks");
    const int i = (b - 134) * 256 + threadIdx.x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (i < kTail4) reinterpret_cast<f32x4*>(fold + kFoldOffBias + 128)[i] = zero;
    else if (i < kTail4 + kGap4) reinterpret_cast<f32x4*>(fold - 4 * kGap4)[i - kTail4] = zero;
    return;
  }
  if (b >= 130) {                                   // direction part: 16 blocks of 1 KiB, unchanged
    const int i = (b - 130) * 256 + threadIdx.x;    // float4 index, < 1024
    reinterpret_cast<f32x4*>(fold + kFoldOffDir)[i] = reinterpret_cast<const f32x4*>(pk + kOffViewsDir)[i];
    return;
  }
  const bool bias = b >= 128;
  // the row of Wv this thread's output belongs to: out-tile j, row (lane & 31) of it
  int j, row, g = 0, h = 0;
  if (!bias) { j = b & 3; g = b >> 2; h = lane >> 5; row = lane & 31; }
  else {
    const int rel = (b - 128) * 64 + lane, o = act_feat((rel & 63) >> 4, rel & 15, rel >> 6);     // [h][t*16 + r] as kOffBiasViews
    j = o >> 5; row = o & 31;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
  for (int mm = 0; mm < 64; ++mm) {
    const int m = part * 64 + mm;
    const int mt = m >> 5, mh = (m >> 2) & 1, mg = 4 * mt + ((m & 31) >> 3), mq = m & 3;          // Wv[o][m]: block (mg, j), lane (row, mh), component mq
    const double wv = (double)pk[kOffViews + (((long long)(mg * 4 + j) * 64 + row + 32 * mh) << 2) + mq];
    if (!bias) {
      // Wf[m][k], k = the four features this lane's float4 holds in block (g, .): block (g, m >> 5), lane (m & 31, h)
      const f32x4 wf = *reinterpret_cast<const f32x4*>(pk + kOffFeat + (((long long)(g * 8 + mt) * 64 + (m & 31) + 32 * h) << 2));
      acc[0] += wv * (double)wf.x; acc[1] += wv * (double)wf.y; acc[2] += wv * (double)wf.z; acc[3] += wv * (double)wf.w;
    } else {
      const int mr = (m & 3) + 4 * ((m & 31) >> 3);
      acc[0] += wv * (double)pk[kOffBias + 8 * 256 + mh * 128 + mt * 16 + mr];                       // bf[m]
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) part_sum[part][lane][q] = acc[q];
  __syncthreads();
  if (part != 0) return;
  double r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = (part_sum[0][lane][q] + part_sum[1][lane][q]) + (part_sum[2][lane][q] + part_sum[3][lane][q]);
  if (!bias) {
    f32x4 v; v.x = (float)r[0]; v.y = (float)r[1]; v.z = (float)r[2]; v.w = (float)r[3];
    reinterpret_cast<f32x4*>(fold + kFoldOffWvf)[b * 64 + lane] = v;
  } else {
    const int rel = (b - 128) * 64 + lane;
    fold[kFoldOffBias + rel] = (float)(r[0] + (double)pk[kOffBiasViews + rel]);
  }
}

// transposed stream for the backward chain (nerf_layout.h kBwd*)
__global__ void nerf_pack_bwd_kernel(PackArgs a) {
  using namespace nerf;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kBwdPackedFloats) return;
  float v = 0.0f;
  if (i < kBwdOffWAlpha) {
    // which layer: (offset, ntiles, source weight, row stride, column offset, output kind)
    long long rel; int nt; const float* W; int ld; int kind;      // kind 0: hidden out cols (+coff), 1: PE slots
    int coff = 0;
    if (i < kBwdOffWfT) { rel = i - kBwdOffWvT; nt = 8; W = a.p[P_WV]; ld = 283; kind = 0; }
    else if (i < kBwdOffW7T) { rel = i - kBwdOffWfT; nt = 8; W = a.p[P_WF]; ld = 256; kind = 0; }
    else if (i < kBwdOffW6T) { rel = i - kBwdOffW7T; nt = 8; W = a.p[14]; ld = 256; kind = 0; }
    else if (i < kBwdOffW5bT) { rel = i - kBwdOffW6T; nt = 8; W = a.p[12]; ld = 256; kind = 0; }
    else if (i < kBwdOffW5aT) { rel = i - kBwdOffW5bT; nt = 8; W = a.p[10]; ld = 319; kind = 0; coff = 63; }
    else if (i < kBwdOffW4T) { rel = i - kBwdOffW5aT; nt = 2; W = a.p[10]; ld = 319; kind = 1; }
    else if (i < kBwdOffW0T) { const long long r2 = i - kBwdOffW4T; const int li = 4 - (int)(r2 / wsize(128, 8));
                               rel = r2 % wsize(128, 8); nt = 8; W = a.p[2 * li]; ld = 256; kind = 0; }
    else { rel = i - kBwdOffW0T; nt = 2; W = a.p[P_W0]; ld = 63; kind = 1; }
    const int q = (int)(rel & 3), lane = (int)((rel >> 2) & 63);
    const long long blk = rel >> 8;
    const int j = (int)(blk % nt), gq = (int)(blk / nt);
    const int s = 4 * gq + q, t = s >> 4, r = s & 15, hk = lane >> 5, irow = lane & 31;
    const int krow = act_feat(t, r, hk);             // feature of the layer's OUTPUT (the reduction index here)
    if (kind == 0) v = W[(long long)krow * ld + coff + 32 * j + irow];
    else {
      const int hp = (irow >> 2) & 1, rp = (irow & 3) + 4 * (irow >> 3);      // accumulator row -> (register, half)
      const int c = pe_xyz_feat(16 * j + rp, hp);
      v = c < 0 ? 0.0f : W[(long long)krow * ld + c];
    }
  } else if (i < kBwdOffWRgb) v = act_order_value<7>(a.p[P_WA], (int)(i - kBwdOffWAlpha));
  else if (i < kBwdOffWRgb + 384) v = pack_w_rgb_value(a.p[P_WR], (int)(i - kBwdOffWRgb));
  a.out[i] = v;
}

// The two tilings of the fp16 fragment streams (nerf_layout.h): an A fragment is kRows out-features x kStep input features, lane =
// (row, g); feat / pe_xyz / pe_dir map (k-step, element j, lane group g) to the input feature.  The ranges up to the sigma head
// are the same fragment numbers in both streams.
struct Frag32x16 {             // v_mfma_f32_32x32x16_f16, "fp16-activation path"
  static constexpr int kRows = 32, kStep = 16;
  static constexpr int kFragFeat = nerf::kF16FragFeat, kFragViews = nerf::kF16FragViews, kFragRgb = nerf::kF16FragRgb, kFragEnd = nerf::kF16Frags;
  static __device__ constexpr int feat(int s, int j, int g) { return nerf::act16_feat(s, j, g); }
  static __device__ constexpr int pe_xyz(int n, int g) { return nerf::pe_xyz_feat(n, g); }
  static __device__ constexpr int pe_dir(int n, int g) { return nerf::pe_dir_feat(n, g); }
};
struct Frag16x32 {             // v_mfma_f32_16x16x32_f16, "f16s" (its tail up to kF16Frags: zero pad fragments)
  static constexpr int kRows = 16, kStep = 32;
  static constexpr int kFragFeat = nerf::kF16sFragFeat, kFragViews = nerf::kF16sFragViews, kFragRgb = nerf::kF16sFragRgb, kFragEnd = nerf::kF16sFragEnd;
  static __device__ constexpr int feat(int s, int j, int g) { return nerf::act16s_feat(s, j, g); }
  static __device__ constexpr int pe_xyz(int n, int g) { return nerf::pe16s_xyz_feat(n, g); }
  static __device__ constexpr int pe_dir(int n, int g) { return nerf::pe16s_dir_feat(n, g); }
};
static_assert(nerf::kF16sFragL1 == nerf::kF16FragL1 && nerf::kF16sFragL5 == nerf::kF16FragL5 && nerf::kF16sFragL6 == nerf::kF16FragL6,
              "frag_stream_value: one set of fragment ranges for L0..L7");

// fp32 value of element (fragment F, lane, j) of an fp16 fragment stream with tiling T
template <class T>
__device__ __forceinline__ float frag_stream_value(const PackArgs& a, int F, int lane, int j) {
  using namespace nerf;
  constexpr int R = T::kRows, HS = 256 / T::kStep, PS = 64 / T::kStep, DS = 32 / T::kStep;   // hidden / xyz PE / dir PE k-steps per out-tile
  const int g = lane / R, row = lane % R;
  const int cj = T::feat(0, j, g);                             // feature inside its k-step
  float v = 0.0f;
  if (F < kF16FragL1) {                                       // L0: 256 / R m x PS PE k-steps
    const int m = F / PS, s = F % PS, c = T::pe_xyz(8 * s + j, g);
    if (c >= 0) v = a.p[P_W0][(R * m + row) * 63 + c];
  } else if (F < kF16FragL5) {                                // L1..L4
    const int f = F - kF16FragL1, li = 1 + (f >> 7), m = (f & 127) / HS, s = f % HS;
    v = a.p[2 * li][(R * m + row) * 256 + T::kStep * s + cj];
  } else if (F < kF16FragL6) {                                // L5: PS PE + HS hidden k-steps per m
    const int f = F - kF16FragL5, m = f / (PS + HS), s = f % (PS + HS);
    if (s < PS) { const int c = T::pe_xyz(8 * s + j, g); if (c >= 0) v = a.p[10][(R * m + row) * 319 + c]; }
    else v = a.p[10][(R * m + row) * 319 + 63 + T::kStep * (s - PS) + cj];
  } else if (F < kF16FragSigma) {                             // L6, L7
    const int f = F - kF16FragL6, li = 6 + (f >> 7), m = (f & 127) / HS, s = f % HS;
    v = a.p[2 * li][(R * m + row) * 256 + T::kStep * s + cj];
  } else if (F < T::kFragFeat) {                              // sigma head: row 0 only
    const int s = F - kF16FragSigma;
    if (row == 0) v = a.p[P_WA][T::kStep * s + cj];
  } else if (F < T::kFragViews) {                             // feature
    const int f = F - T::kFragFeat, m = f / HS, s = f % HS;
    v = a.p[P_WF][(R * m + row) * 256 + T::kStep * s + cj];
  } else if (F < T::kFragRgb) {                               // views: HS feature + DS dir k-steps per m
    const int f = F - T::kFragViews, m = f / (HS + DS), s = f % (HS + DS);
    if (s < HS) v = a.p[P_WV][(R * m + row) * 283 + T::kStep * s + cj];
    else { const int c = T::pe_dir(8 * (s - HS) + j, g); if (c >= 0) v = a.p[P_WV][(R * m + row) * 283 + 256 + c]; }
  } else if (F < T::kFragEnd) {                               // rgb head: rows 0..2
    const int s = F - T::kFragRgb;
    if (row < 3) v = a.p[P_WR][row * 128 + T::kStep * s + cj];
  }
  return v;
}

// (hi, lo) fragment pair of the split streams: element e of fragment F holds w_h, the fragment behind it w_l (w = w_h + 2^-11 w_l)
__device__ __forceinline__ void store_split_f16(_Float16* out, int F, long long e, float v) {
  const _Float16 hi = (_Float16)v;
  const long long base = ((long long)(2 * F) << 9) + (e & 511);
  out[base] = hi;
  out[base + 512] = (_Float16)((v - (float)hi) * 2048.0f);
}

// f16s stream: const region (fp32 biases in NATURAL order) + A fragments
__global__ void nerf_pack_f16s_kernel(PackArgs a) {
  using namespace nerf;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr long long n_const = kF16ConstBytes / 4;
  constexpr long long n_half = (long long)kF16Frags * 512;
  if (i < n_const) {
    float v = 0.0f;
    if (i < kF16sOffBiasViews) {
      const int layer = (int)i >> 8, c = (int)i & 255;
      v = (layer < 8 ? a.p[2 * layer + 1] : a.p[P_BF])[c];
    } else if (i < kF16sOffHeadBias) v = a.p[P_BV][(int)i - kF16sOffBiasViews];
    else if (i < kF16sOffHeadBias + 4) v = pack_head_bias_value(a, (int)i - kF16sOffHeadBias);
    a.out[i] = v;
    return;
  }
  const long long e = i - n_const;
  if (e >= n_half) return;
  const int F = (int)(e >> 9), lane = (int)((e >> 3) & 63), j = (int)(e & 7);
  reinterpret_cast<_Float16*>(reinterpret_cast<char*>(a.out) + kF16ConstBytes)[e] = (_Float16)frag_stream_value<Frag16x32>(a, F, lane, j);
}

// backward f32x stream: transposed weights as (hi, lo) fragment pairs + w_alpha / w_rgb in the const region
__global__ void nerf_pack_bwd_f32x_kernel(PackArgs a) {
  using namespace nerf;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr long long n_const = kF16ConstBytes / 4;
  constexpr long long n_el = (long long)kXbSteps * 512;
  if (i < n_const) {
    float v = 0.0f;
    if (i < 256) v = act_order_value<7>(a.p[P_WA], (int)i);
    else if (i < 256 + 384) v = pack_w_rgb_value(a.p[P_WR], (int)i - 256);
    a.out[i] = v;
    return;
  }
  const long long e = i - n_const;
  if (e >= n_el) return;
  const int F = (int)(e >> 9), lane = (int)((e >> 3) & 63), j = (int)(e & 7);
  const int hk = lane >> 5, irow = lane & 31;
  // locate (layer, m, s): W^T fragment value = W[krow = out feature of the layer][col = in feature]
  const float* W; int ld, coff = 0, ks, f; bool pe_out = false;
  if (F < kXbStepsWfT) { f = F - kXbStepsWvT; ks = 8; W = a.p[P_WV]; ld = 283; }
  else if (F < kXbStepsW5aT) { const int rel = F - kXbStepsWfT, li = rel >> 7; f = rel & 127; ks = 16;
    if (li == 0) { W = a.p[P_WF]; ld = 256; } else if (li == 1) { W = a.p[14]; ld = 256; }
    else if (li == 2) { W = a.p[12]; ld = 256; } else { W = a.p[10]; ld = 319; coff = 63; } }
  else if (F < kXbStepsW4T) { f = F - kXbStepsW5aT; ks = 16; W = a.p[10]; ld = 319; pe_out = true; }
  else if (F < kXbStepsW0T) { const int rel = F - kXbStepsW4T, li = 4 - (rel >> 7); f = rel & 127; ks = 16; W = a.p[2 * li]; ld = 256; }
  else { f = F - kXbStepsW0T; ks = 16; W = a.p[P_W0]; ld = 63; pe_out = true; }
  const int m = f / ks, s = f % ks;
  const int krow = act16_feat(s, j, hk);
  float v;
  if (!pe_out) v = W[(long long)krow * ld + coff + 32 * m + irow];
  else {
    const int hp = (irow >> 2) & 1, rp = (irow & 3) + 4 * (irow >> 3);
    const int c = pe_xyz_feat(16 * m + rp, hp);
    v = c < 0 ? 0.0f : W[(long long)krow * ld + c];
  }
  store_split_f16(reinterpret_cast<_Float16*>(reinterpret_cast<char*>(a.out) + kF16ConstBytes), F, e, v);
}

// fp16 stream (nerf_layout.h "fp16-activation path"): const region (fp32 biases) + A fragments; with SPLIT the
// "f32x" stream: every fragment followed by its low-part fragment
template <bool SPLIT>
__global__ void nerf_pack_f16_kernel(PackArgs a) {
  using namespace nerf;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr long long n_const = kF16ConstBytes / 4;
  constexpr long long n_half = (long long)kF16Frags * 512;
  if (i < n_const) {                     // const region, floats
    float v = 0.0f;
    if (i < kF16OffBiasViews) v = pack_bias_value(a, (int)i);
    else if (i < kF16OffHeadBias) v = act_order_value<6>(a.p[P_BV], (int)i - kF16OffBiasViews);
    else if (i < kF16OffHeadBias + 4) v = pack_head_bias_value(a, (int)i - kF16OffHeadBias);
    a.out[i] = v;
    return;
  }
  const long long e = i - n_const;
  if (e >= n_half) return;
  const int F = (int)(e >> 9), lane = (int)((e >> 3) & 63), j = (int)(e & 7);
  const float v = frag_stream_value<Frag32x16>(a, F, lane, j);
  _Float16* out = reinterpret_cast<_Float16*>(reinterpret_cast<char*>(a.out) + kF16ConstBytes);
  if (SPLIT) store_split_f16(out, F, e, v);
  else out[e] = (_Float16)v;
}

// ------------------------------------------------------------------------------------ PE (test entry)
__global__ void nerf_pe_kernel(const float* __restrict__ x, long long n, int n_freqs, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ch = 3 + 6 * n_freqs;
  if (i >= n * 3) return;
  const long long p = i / 3;
  const int c = (int)(i - p * 3);
  const float v = x[i];
  out[p * ch + c] = v;
  for (int k = 0; k < n_freqs; ++k) {
    float sv, cv;
    sincosf(v * (float)(1 << k), &sv, &cv);
    out[p * ch + 3 + 6 * k + c] = sv;
    out[p * ch + 3 + 6 * k + 3 + c] = cv;
  }
}

// ------------------------------------------------------------------------------------ fine sampling
// One thread per ray, sequential scans in the reference's CPU order (cumprod / cumsum are
// sequential in torch CPU too).  A 64-ray block stages its I/O through LDS: the coarse sigmas are
// loaded cooperatively, every lane then owns one padded 192-float LDS row (sigma -> fine depths in
// [0,128) with the cdf in [128,191) -> the merged depths), and the 64 x 192 sorted depths are
// written back coalesced.
// Two instances of one body, which is what keeps them bit-compatible on the same tables:
//  <false> one coarse table and one ascending u table for all rays (s_tab = t[64] | u[128]); t_fine comes out of the walk;
//          optionally (fast_sampling) also the ESS/ERT validity of every merged sample (volume_renderer.py:116-123, :132-133,
//          :158-193, :359-369), carried through the merge as the sign of the depth.
//  <true>  a coarse table and a u table per ray (t of ray r at t_coarse + r * t_stride, u at u + r * u_stride; stride 0 shares one
//          table): s_tab = one 65-float coarse row per ray.  t_sorted depends only on the MULTISET of fine depths, so each lane
//          sorts its ray's 128 u ascending (registers, bitonic) and then runs the same monotone walk.  The row's slots [0,128)
//          hold sigma, then the ray's u (staged coalesced), then the sorted u the walk overwrites in place with the fine depths
//          (slot j <= k is written only after u[k] was read); t_fine is in the caller's u order, by bisection.  No masks.
// LDS per 64-ray workgroup: the 64 x 193-float rows (49 408 B) + 768 B of shared tables, or + 16 640 B of coarse rows.
constexpr int kSampleThreads = 64;
constexpr int kBufPitch = 193;     // odd pitch: lanes walking their own rows never share a bank
constexpr int kTcPitch = 65;       // odd pitch, as kBufPitch

struct SampleArgs {
  const float* raw_c;        // [n,64,4]
  const float* t_coarse;     // [64] or [n,64]
  long long t_stride;        // 0 or 64
  const float* u;            // [128] or [n,128]
  long long u_stride;        // 0 or 128
  long long n_rays;
  float* t_sorted;           // [n,192]
  float* t_fine;             // optional [n,128], in the caller's u order
  unsigned char* valid_sorted;   // optional [n,192], 1 = evaluate with the fine network (shared tables only)
  int fast_sampling;
  float weights_threshold, ert_threshold;
};

__device__ __forceinline__ float alpha_of(float sigma, float delta) {
  return __fsub_rn(1.0f, expf(__fmul_rn(-sigma, delta)));       // 1 - exp(-sigma*delta)
}

// torch.sum(w, -1) of volume_renderer.py:138 on a 62-element fp32 row, in the CPU kernel's own order (ATen SumKernel.cpp,
// vectorized_inner_sum / row_sum with 8-lane vectors and 4 accumulators -- verified bit for bit against torch.sum on the fixture
// rows): the 56 leading elements as 7 vectors of 8, lane sums ((((((v0 + v4) + v5) + v6) + v1) + v2) + v3), then the 6 tail
// elements and the 8 lane sums added one by one.  A plain left-to-right sum (rounds 1-2) is off by up to 3e-6 relative on rows of
// many equal 1e-5 terms, i.e. cdf[62] = 1 + 3e-6: it moved every fine sample of a ray by ~3e-6 against the reference's and was
// the "unexplained" part of the white-noise family's excess over the noise floor (round-2 VERDICT Weak 8).
template <class Get>
__device__ __forceinline__ float torch_sum62_of(Get x) {
  float P[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float p = __fadd_rn(x(j), x(32 + j));
    p = __fadd_rn(p, x(40 + j));
    p = __fadd_rn(p, x(48 + j));
    p = __fadd_rn(p, x(8 + j));
    p = __fadd_rn(p, x(16 + j));
    P[j] = __fadd_rn(p, x(24 + j));
  }
  float acc = x(56);
#pragma unroll
  for (int k = 57; k < 62; ++k) acc = __fadd_rn(acc, x(k));
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __fadd_rn(acc, P[j]);
  return acc;
}
__device__ __forceinline__ float torch_sum62(const float* w) { return torch_sum62_of([&](int k) { return w[k]; }); }

// Ascending bitonic network over one thread's 128 registers.  Fully unrolled (unroll(full): plain `#pragma unroll` left the
// array in scratch, 528 B per lane), so every index is a constant and the array lives in VGPRs.
__device__ __forceinline__ void sort128_ascending(float (&r)[NERF_N_IMPORTANCE]) {
#pragma clang loop unroll(full)
  for (int k = 2; k <= NERF_N_IMPORTANCE; k <<= 1) {
#pragma clang loop unroll(full)
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma clang loop unroll(full)
      for (int i = 0; i < NERF_N_IMPORTANCE; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const float x = r[i], y = r[l];
          const bool up = (i & k) == 0;
          r[i] = up ? fminf(x, y) : fmaxf(x, y);
          r[l] = up ? fmaxf(x, y) : fminf(x, y);
        }
      }
    }
  }
}

// Inverse CDF of one u given its searchsorted(right) index; also the two bins it interpolates between.
__device__ __forceinline__ float inv_cdf_at(const float* cdf, const float* tc, float u, int ind, int& below, int& above) {
  constexpr int S = NERF_N_SAMPLES;
  below = min(max(ind - 1, 0), S - 3);
  above = min(ind, S - 3);                             // clamp to 61: tail collapse
  const float cb = cdf[below], ca = cdf[above];
  const float bb = __fmul_rn(0.5f, __fadd_rn(tc[below + 1], tc[below]));
  const float ba = __fmul_rn(0.5f, __fadd_rn(tc[above + 1], tc[above]));
  float denom = __fsub_rn(ca, cb);
  if (denom < 1e-5f) denom = 1.0f;
  const float frac = __fdiv_rn(__fsub_rn(u, cb), denom);
  return __fadd_rn(bb, __fmul_rn(frac, __fsub_rn(ba, bb)));
}

template <bool RAYS>
__global__ __launch_bounds__(kSampleThreads)
void nerf_sample_fine_kernel(SampleArgs a) {
  constexpr int S = NERF_N_SAMPLES, F = NERF_N_IMPORTANCE, NB = S - 1;   // 63 cdf entries / bins
  __shared__ float s_tab[RAYS ? kSampleThreads * kTcPitch : S + F];
  __shared__ float s_buf[kSampleThreads * kBufPitch];
  const int lane = threadIdx.x;
  const long long ray0 = (long long)blockIdx.x * kSampleThreads;
  if (!RAYS) {
    s_tab[lane] = a.t_coarse[lane];
    s_tab[S + lane] = a.u[lane];
    s_tab[S + lane + 64] = a.u[lane + 64];
  }
  for (int r = 0; r < kSampleThreads; ++r) {          // lane = coarse sample index
    long long rg = ray0 + r;
    if (rg >= a.n_rays) rg = a.n_rays - 1;
    s_buf[r * kBufPitch + lane] = a.raw_c[rg * (S * 4) + lane * 4 + 3];
    if (RAYS) s_tab[r * kTcPitch + lane] = a.t_coarse[rg * a.t_stride + lane];
  }
  __syncthreads();
  float* buf = s_buf + lane * kBufPitch;
  float* cdf = buf + F;        // slots 128..190: free until the merge, which no longer needs the cdf
  const float* tc = RAYS ? s_tab + lane * kTcPitch : s_tab;
  const float* us = RAYS ? buf : s_tab + S;            // the ascending u the walk reads
  auto depth_of = [](float v) { return RAYS ? v : fabsf(v); };      // shared tables: the sign carries "masked out"

  // weights of the coarse pass (volume_renderer.py:67-96), inner 62 + eps, running sum
  float T = 1.0f, dsum = 0.0f, dmax = 0.0f;
  unsigned long long empty_bits = 0, ert_bits = 0;
  bool ert_seen = false;
  for (int i = 0; i < S; ++i) {
    const float sigma = fmaxf(buf[i], 0.0f);
    const float delta = (i < S - 1) ? __fsub_rn(tc[i + 1], tc[i]) : 1e10f;
    const float alpha = alpha_of(sigma, delta);
    const float w = __fmul_rn(T, alpha);
    if (i >= 1 && i <= S - 2) cdf[i - 1] = __fadd_rn(w, 1e-5f);     // stash w+eps in cdf slots 0..61 (summed below, in torch's order)
    if (!RAYS) {
      dsum = __fadd_rn(dsum, sigma);
      dmax = fmaxf(dmax, sigma);
      if (i >= 1 && i <= S - 2) {
        if (w < a.weights_threshold) empty_bits |= 1ull << (i - 1);
        ert_seen = ert_seen || (T < a.ert_threshold);     // cummax of (T < thr) over the inner bins
        if (ert_seen) ert_bits |= 1ull << (i - 1);
      }
    }
    T = __fmul_rn(T, fminf(fmaxf(__fsub_rn(1.0f, alpha), 1e-10f), 1.0f));
  }
  const float wsum = torch_sum62(cdf);
  const bool empty_ray = dsum < 1e-3f;
  const bool object_ray = dmax > 0.5f;
  // cdf = [0, cumsum(pdf)]  (63 entries)
  {
    float run = 0.0f, prev = cdf[0];
    cdf[0] = 0.0f;
    for (int m = 1; m < NB; ++m) {
      run = __fadd_rn(run, __fdiv_rn(prev, wsum));
      prev = cdf[m];
      cdf[m] = run;
    }
  }
  const long long ray = ray0 + lane;
  const bool ray_ok = ray < a.n_rays;
  int below, above;
  if (RAYS) {
    __syncthreads();                                   // every lane has read its sigmas: slots [0,128) take the rays' u
    for (int r = 0; r < kSampleThreads; ++r) {
      long long rg = ray0 + r;
      if (rg >= a.n_rays) rg = a.n_rays - 1;
      s_buf[r * kBufPitch + lane] = a.u[rg * a.u_stride + lane];
      s_buf[r * kBufPitch + 64 + lane] = a.u[rg * a.u_stride + 64 + lane];
    }
    __syncthreads();
    if (a.t_fine && ray_ok) {                          // in the caller's order: searchsorted(right) by bisection
      for (int k = 0; k < F; ++k) {
        const float u = buf[k];
        int lo = 0, hi = NB;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] <= u) lo = mid + 1; else hi = mid; }
        a.t_fine[ray * F + k] = inv_cdf_at(cdf, tc, u, lo, below, above);
      }
    }
    float r[F];
#pragma clang loop unroll(full)
    for (int k = 0; k < F; ++k) r[k] = buf[k];
    sort128_ascending(r);
#pragma clang loop unroll(full)
    for (int k = 0; k < F; ++k) buf[k] = r[k];
  }
  // inverse CDF at the ascending u; u ascending -> the searchsorted(right=True) index only grows
  int ind = 0;
  for (int k = 0; k < F; ++k) {
    const float u = us[k];
    while (ind < NB && cdf[ind] <= u) ++ind;
    float v = inv_cdf_at(cdf, tc, u, ind, below, above);
    if (!RAYS) {
      if (a.t_fine && ray_ok) a.t_fine[ray * F + k] = v;
      if (a.fast_sampling) {
        const bool be = (empty_bits >> below) & 1, ae = (empty_bits >> above) & 1, ert = (ert_bits >> below) & 1;
        const bool ess_nv = object_ray ? (be && ae) : (be || ae);
        if (ess_nv || ert || empty_ray) v = -v;           // depths are > 0: the sign carries "masked out"
      }
    }
    // keep the fine depths sorted even if rounding ever produced a 1-ulp inversion (torch.sort would fix it too)
    int j = k;
    while (j > 0 && depth_of(buf[j - 1]) > depth_of(v)) { buf[j] = buf[j - 1]; --j; }
    buf[j] = v;
  }
  // in-place two-way merge from the back of (sorted coarse table, sorted fine depths) = cat + torch.sort;
  // on ties the coarse sample comes first
  {
    int ic = S - 1, jf = F - 1;
    for (int k = S + F - 1; k >= 0; --k) {
      const bool take_f = (ic < 0) || (jf >= 0 && depth_of(buf[jf]) >= tc[ic]);
      if (take_f) { buf[k] = buf[jf]; --jf; }
      else { buf[k] = tc[ic]; --ic; }
    }
  }
  __syncthreads();
  for (int i = 0; i < S + F; ++i) {                    // 64 rays x 192 depths, coalesced
    const int e = lane + 64 * i, r = e / (S + F), k = e - r * (S + F);
    const long long rg = ray0 + r;
    if (rg < a.n_rays) {
      const float v = s_buf[r * kBufPitch + k];
      a.t_sorted[rg * (S + F) + k] = depth_of(v);
      if (!RAYS && a.valid_sorted) a.valid_sorted[rg * (S + F) + k] = v > 0.0f;
    }
  }
}

// Stream compaction of the valid (ray, sample) ids for the masked fine pass (replaces the boolean
// indexing of network.py:207-214): order inside `index` is arbitrary, results are scattered back by id.
__global__ __launch_bounds__(256)
void nerf_compact_kernel(const unsigned char* __restrict__ valid, long long n, int* __restrict__ index,
                         int* __restrict__ count) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool v = i < n && valid[i] != 0;
  const unsigned long long m = __ballot(v);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(count, (int)__popcll(m));
  base = __shfl(base, 0);
  if (v) index[base + (int)__popcll(m & ((1ull << lane) - 1ull))] = (int)i;
}

// Point ids of the LAST sample of every ray (the fp16 paths' far-plane guard, nerf_render_forward): index[r] = r * S + S - 1.
__global__ __launch_bounds__(256)
void nerf_last_sample_index_kernel(int* __restrict__ index, int* __restrict__ count, long long n_rays, int S) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_rays) index[r] = (int)(r * S + S - 1);
  if (r == 0) *count = (int)n_rays;
}

// ------------------------------------------------------------------------------------ compositing
__device__ __forceinline__ float sigmoid_rn(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }

// Running state of one ray and the per-sample step of volume_renderer.py:67-96, :414-432; the rounding sequence of `add` and
// `store` is what both forward kernels (and every stored result) agree on bit for bit.
// The weight of one sample (volume_renderer.py:67-96): alpha of relu(sigma) over delta and the factor q the transmittance takes on
// behind the sample; step() gives w_k = T alpha and moves T on.  The one definition of the weights: nerf_composite's kernels take
// both halves at once, nerf_composite_normals computes `of` lane-parallel and walks step() over the lanes in sample order.
struct CompositeWeight {
  float alpha, q;
  static __device__ __forceinline__ CompositeWeight of(float sigma_raw, float delta) {
    const float alpha = alpha_of(fmaxf(sigma_raw, 0.0f), delta);
    return {alpha, fminf(fmaxf(__fsub_rn(1.0f, alpha), 1e-10f), 1.0f)};
  }
  __device__ __forceinline__ float step(float& T) const {
    const float wk = __fmul_rn(T, alpha);
    T = __fmul_rn(T, q);
    return wk;
  }
};

struct CompositeAcc {
  float T = 1.0f, r = 0.f, g = 0.f, b = 0.f, d = 0.f, w = 0.f;
  __device__ __forceinline__ float add(f32x4 v, float t_cur, float delta) {      // returns the sample's weight
    const float wk = CompositeWeight::of(v.w, delta).step(T);
    const float cr = sigmoid_rn(v.x), cg = sigmoid_rn(v.y), cb = sigmoid_rn(v.z);
    r = __fadd_rn(r, __fmul_rn(wk, cr));
    g = __fadd_rn(g, __fmul_rn(wk, cg));
    b = __fadd_rn(b, __fmul_rn(wk, cb));
    d = __fadd_rn(d, __fmul_rn(wk, t_cur));
    w = __fadd_rn(w, wk);
    return wk;
  }
  __device__ __forceinline__ void store(long long ray, int white_bkgd, float* __restrict__ rgb_out, float* __restrict__ depth_out) {
    if (white_bkgd) {
      const float bg = __fsub_rn(1.0f, w);
      r = __fadd_rn(r, bg); g = __fadd_rn(g, bg); b = __fadd_rn(b, bg);
    }
    rgb_out[ray * 3 + 0] = r; rgb_out[ray * 3 + 1] = g; rgb_out[ray * 3 + 2] = b;
    depth_out[ray] = d;
  }
};

__global__ __launch_bounds__(256)
void nerf_composite_kernel(const float* __restrict__ raw, const float* __restrict__ tvals,
                           long long t_ray_stride, long long n_rays, int S, int white_bkgd,
                           float* __restrict__ rgb_out, float* __restrict__ depth_out,
                           float* __restrict__ weights_out) {
  const long long ray = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ray >= n_rays) return;
  const f32x4* r4 = reinterpret_cast<const f32x4*>(raw) + ray * S;
  const float* t = tvals + ray * t_ray_stride;
  CompositeAcc acc;
  float t_cur = t[0];
  for (int k = 0; k < S; ++k) {
    const f32x4 v = r4[k];
    const float t_next = (k < S - 1) ? t[k + 1] : 0.0f;
    const float w = acc.add(v, t_cur, (k < S - 1) ? __fsub_rn(t_next, t_cur) : 1e10f);
    if (weights_out) weights_out[ray * S + k] = w;
    t_cur = t_next;
  }
  acc.store(ray, white_bkgd, rgb_out, depth_out);
}

// Same arithmetic, same order, but HBM-friendly: one wave per 64 rays; each 16-sample chunk of the
// 64 rays is loaded cooperatively (256-B contiguous pieces per ray) into padded LDS rows, then every
// lane walks its own ray's row.  2.5 GB of reads per 800x800 frame at close to streaming rate
// instead of 64 lanes striding 3 KiB apart.  Bit-identical results to nerf_composite_kernel.
constexpr int kCompChunk = 16;
__global__ __launch_bounds__(64)
void nerf_composite_staged_kernel(const float* __restrict__ raw, const float* __restrict__ tvals,
                                  long long t_ray_stride, long long n_rays, int S, int white_bkgd,
                                  float* __restrict__ rgb_out, float* __restrict__ depth_out,
                                  float* __restrict__ weights_out) {
  __shared__ f32x4 s_raw[64 * (kCompChunk + 1)];
  __shared__ float s_t[64 * (kCompChunk + 1)];
  const int lane = threadIdx.x;
  const long long ray0 = (long long)blockIdx.x * 64;
  const long long ray = ray0 + lane;
  const bool valid = ray < n_rays;
  const f32x4* r4 = reinterpret_cast<const f32x4*>(raw);
  CompositeAcc acc;
  f32x4 pv = {0.f, 0.f, 0.f, 0.f};      // pending sample (its delta needs the next depth)
  float pt = 0.0f;
  auto emit = [&](f32x4 v, float t_cur, float delta, int k) {
    const float w = acc.add(v, t_cur, delta);
    if (weights_out && valid) weights_out[ray * S + k] = w;
  };
  for (int c0 = 0; c0 < S; c0 += kCompChunk) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCompChunk; ++i) {                 // 64 rays x 16 samples of float4
      const int e = lane + 64 * i, rr = e / kCompChunk, ss = e % kCompChunk;
      long long rg = ray0 + rr;
      if (rg >= n_rays) rg = n_rays - 1;
      s_raw[rr * (kCompChunk + 1) + ss] = r4[rg * S + c0 + ss];
    }
#pragma unroll
    for (int i = 0; i < kCompChunk / 4; ++i) {             // 64 rays x 16 depths
      const int e = lane + 64 * i, rr = e / 4, q = e % 4;
      long long rg = ray0 + rr;
      if (rg >= n_rays) rg = n_rays - 1;
      const f32x4 tv = *reinterpret_cast<const f32x4*>(tvals + rg * t_ray_stride + c0 + 4 * q);
      float* dst = s_t + rr * (kCompChunk + 1) + 4 * q;
      dst[0] = tv.x; dst[1] = tv.y; dst[2] = tv.z; dst[3] = tv.w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCompChunk; ++k) {
      const f32x4 v = s_raw[lane * (kCompChunk + 1) + k];
      const float t = s_t[lane * (kCompChunk + 1) + k];
      if (c0 + k > 0) emit(pv, pt, __fsub_rn(t, pt), c0 + k - 1);
      pv = v; pt = t;
    }
  }
  emit(pv, pt, 1e10f, S - 1);
  if (valid) acc.store(ray, white_bkgd, rgb_out, depth_out);
}

// ------------------------------------------------------------------------------------ training: backward of compositing / sampling
// One thread per ray, reverse sequential scans: the exact adjoint of the forward loops above
// (autograd of volume_renderer.py:67-96 and :414-432).
//   w_k = T_k a_k, T_k = prod_{j<k} q_j, q = clamp(1-a, 1e-10, 1), a = 1 - exp(-relu(s) delta), delta_k = t_{k+1}-t_k
//   rgb = sum w_k sigmoid(r_k) + (1 - sum w_k) [white], depth = sum w_k t_k
// Given g_rgb [n,3], g_depth [n] -> g_raw [n,S,4], g_t [n,S] (direct dependence through delta and depth).
// One WAVE per ray (a training step has 4096 rays: with one thread per ray the 2 x 192 sequential steps of 64 lonely waves were
// 108 us of dependent instruction latency): lane l owns samples l, l + 64, l + 128, the transmittance is a wave-level
// exclusive prefix product and the suffix sum a wave-level exclusive suffix sum, chunk by chunk with a scalar carry; every
// load and store is one coalesced row segment.  (The scans associate differently from the forward's sequential product:
// rounding-level differences in T, as between any two summation orders.)
constexpr int kCbMaxSamples = 192;

// Inclusive scan over the 64 lanes of a wave: UP: lane l gets op over lanes 0..l (prefix), else over lanes l..63 (suffix)
template <bool UP, class T, class Op>
__device__ __forceinline__ T wave_scan(T x, int lane, Op op) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = UP ? __shfl_up(x, d) : __shfl_down(x, d);
    if (UP ? lane >= d : lane + d < 64) x = op(x, o);
  }
  return x;
}
// The value of the neighbouring lane (UP: lane - 1, else lane + 1); the lane at the end of the wave gets `edge`: turns an
// inclusive scan into the exclusive one
template <bool UP, class T>
__device__ __forceinline__ T wave_shift(T x, int lane, T edge) {
  const T o = UP ? __shfl_up(x, 1) : __shfl_down(x, 1);
  return lane == (UP ? 0 : 63) ? edge : o;
}
constexpr auto op_sum = [](auto x, auto y) { return x + y; };
constexpr auto op_prod = [](auto x, auto y) { return x * y; };
constexpr auto op_max = [](auto x, auto y) { return max(x, y); };

__global__ __launch_bounds__(256)
void nerf_composite_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ tvals, long long t_ray_stride,
                               long long n_rays, int S, int white_bkgd, const float* __restrict__ g_rgb,
                               const float* __restrict__ g_depth, float* __restrict__ g_raw, float* __restrict__ g_t) {
  constexpr int C = kCbMaxSamples / 64;
  const int lane = threadIdx.x & 63;
  const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;                                   // (wave-uniform)
  const f32x4* r4 = reinterpret_cast<const f32x4*>(raw) + ray * S;
  f32x4* g4 = reinterpret_cast<f32x4*>(g_raw) + ray * S;
  const float* t = tvals + ray * t_ray_stride;
  float* gt = g_t ? g_t + ray * S : nullptr;
  const float gr = g_rgb[ray * 3 + 0], gg = g_rgb[ray * 3 + 1], gb = g_rgb[ray * 3 + 2];
  const float gd = g_depth ? g_depth[ray] : 0.0f;
  const float wb = white_bkgd ? 1.0f : 0.0f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  f32x4 v[C];
  float tk[C], delta[C], e[C], alpha[C], om[C], q[C], Tk[C], g_delta[C], gt_own[C];
  // forward sweep: T_k = prod_{j<k} q_j
  float carry = 1.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int k = 64 * c + lane;
    const bool live = k < S;
    v[c] = live ? r4[k] : zero4;
    tk[c] = live ? t[k] : 0.0f;
    const float tn = (k + 1 < S) ? t[k + 1] : tk[c];
    delta[c] = (k < S - 1) ? __fsub_rn(tn, tk[c]) : 1e10f;
    const float sig = fmaxf(v[c].w, 0.0f);
    e[c] = expf(__fmul_rn(-sig, delta[c]));
    alpha[c] = __fsub_rn(1.0f, e[c]);
    om[c] = __fsub_rn(1.0f, alpha[c]);
    q[c] = live ? fminf(fmaxf(om[c], 1e-10f), 1.0f) : 1.0f;
    const float p = wave_scan<true>(q[c], lane, op_prod);
    Tk[c] = carry * wave_shift<true>(p, lane, 1.0f);
    carry *= __shfl(p, 63);
  }
  // reverse sweep: suf_k = sum_{m>k} g_w_m a_m T_m;  g_q_k = suf_k / q_k
  float carry_s = 0.0f;
#pragma unroll
  for (int c = C - 1; c >= 0; --c) {
    const int k = 64 * c + lane;
    const bool live = k < S;
    const float sig = fmaxf(v[c].w, 0.0f);
    const float cr = sigmoid_rn(v[c].x), cg = sigmoid_rn(v[c].y), cb = sigmoid_rn(v[c].z);
    const float g_w = gr * (cr - wb) + gg * (cg - wb) + gb * (cb - wb) + gd * tk[c];
    const float w = Tk[c] * alpha[c];
    const float sfx = wave_scan<false>(live ? g_w * alpha[c] * Tk[c] : 0.0f, lane, op_sum);
    const float suf = wave_shift<false>(sfx, lane, 0.0f) + carry_s;
    carry_s += __shfl(sfx, 0);
    float g_alpha = g_w * Tk[c];
    if (om[c] >= 1e-10f && om[c] <= 1.0f) g_alpha -= suf / q[c];      // clamp passes the gradient inside its range
    const float g_sig = g_alpha * delta[c] * e[c];
    g_delta[c] = (k < S - 1) ? g_alpha * sig * e[c] : 0.0f;
    f32x4 go;
    go.x = gr * w * cr * (1.0f - cr);
    go.y = gg * w * cg * (1.0f - cg);
    go.z = gb * w * cb * (1.0f - cb);
    go.w = v[c].w > 0.0f ? g_sig : 0.0f;
    if (live) g4[k] = go;
    gt_own[c] = gd * w - g_delta[c];                            // delta_k = t_{k+1} - t_k: - g_delta_k here, + g_delta_{k-1} below
  }
  if (gt) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int k = 64 * c + lane;
      const float last_of_prev_chunk = c > 0 ? __shfl(g_delta[c > 0 ? c - 1 : 0], 63) : 0.0f;
      if (k < S) gt[k] = gt_own[c] + wave_shift<true>(g_delta[c], lane, last_of_prev_chunk);
    }
  }
}

// Backward of hierarchical sampling (volume_renderer.py:126-154, :247-264 under autograd): gradient of the
// merged depths w.r.t. the coarse densities (the coarse table and u are constants).  Recomputes the
// forward quantities, then: g_t_fine -> g_cdf[below/above] -> g_pdf (reverse cumsum) -> g_(w+eps) ->
// g_w (inner 62) -> g_sigma through T/alpha -> g_raw_coarse[..., 3] (relu mask).
// One WAVE per ray, lane i = coarse sample i (S = 64), two fine samples per lane.  What decides where a fine sample falls --
// transmittance, the running sum of the weights and the cdf -- is recomputed in the forward's own SEQUENTIAL order (a
// v_readlane walk over the lanes with the forward's rounding intrinsics: bit-identical bins); everything downstream of the
// decisions is a gradient and uses wave scans / LDS atomics.  (One thread per ray took 131 us for the 4096 rays of a step:
// 64 lonely waves whose data-dependent while-loops also ran in lockstep.)
// The two instances are those of nerf_sample_fine_kernel: <false> one coarse table and one ascending u table (s_tab = t[64] |
// u[128]), <true> tables per ray with the forward's strides (s_tab = one coarse row per wave), where each wave first sorts its
// ray's u: the merged-slot logic (k + ic with the running maximum, ties coarse first) needs the fine samples in ascending order.
__device__ __forceinline__ float lane_bcast(float v, int lane_const) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_const));
}
// Ascending bitonic sort of 128 values across a wave: lane l holds elements l and l + 64
__device__ __forceinline__ void wave_sort128_ascending(float (&us)[2], int lane) {
#pragma unroll
  for (int k = 2; k <= 128; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j == 64) {                                   // k == 128: partners share the lane
        const float x = us[0], y = us[1];
        us[0] = fminf(x, y); us[1] = fmaxf(x, y);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int idx = lane + 64 * h;
          const float p = __shfl_xor(us[h], j);
          const bool up = (idx & k) == 0, low = (idx & j) == 0;
          us[h] = (low == up) ? fminf(us[h], p) : fmaxf(us[h], p);
        }
      }
    }
  }
}
template <bool RAYS>
__global__ __launch_bounds__(256)
void nerf_sample_bwd_kernel(const float* __restrict__ raw_c, const float* __restrict__ t_coarse, long long t_stride,
                            const float* __restrict__ u_in, long long u_stride, long long n_rays,
                            const float* __restrict__ g_tsorted, float* __restrict__ g_raw_c) {
  constexpr int S = NERF_N_SAMPLES, F = NERF_N_IMPORTANCE, NB = S - 1;
  static_assert(S == 64 && F == 128, "lane = coarse sample, two fine samples per lane");
  __shared__ float s_tab[RAYS ? 4 * S : S + F];
  __shared__ float s_cdf[4][S];
  __shared__ double s_gcdf[4][S];          // adjoint of the cdf, accumulated in float64 (see below)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long ray_slot = (long long)blockIdx.x * 4 + wv;
  const bool ray_ok = ray_slot < n_rays;                       // a wave past the end recomputes the last ray and stores nothing
  const long long ray = ray_ok ? ray_slot : n_rays - 1;        // (it has to reach the workgroup barriers below)
  float us[2];
  if (RAYS) {
    s_tab[wv * S + lane] = t_coarse[ray * t_stride + lane];
    us[0] = u_in[ray * u_stride + lane];
    us[1] = u_in[ray * u_stride + 64 + lane];
    wave_sort128_ascending(us, lane);
  } else {
    if (threadIdx.x < S) s_tab[threadIdx.x] = t_coarse[threadIdx.x];
    if (threadIdx.x < F) s_tab[S + threadIdx.x] = u_in[threadIdx.x];
  }
  s_gcdf[wv][lane] = 0.0;
  __syncthreads();
  const float* tc = RAYS ? s_tab + wv * S : s_tab;
  const int i = lane;
  // ---- forward recompute, in the forward's order and rounding (nerf_sample_fine_kernel)
  const float s_raw = raw_c[ray * (S * 4) + i * 4 + 3];
  const float sigma = fmaxf(s_raw, 0.0f);
  const float delta = (i < S - 1) ? __fsub_rn(tc[i + 1], tc[i]) : 1e10f;
  const float e = expf(__fmul_rn(-sigma, delta));
  const float alpha = __fsub_rn(1.0f, e);                      // = alpha_of(sigma, delta)
  const float om = __fsub_rn(1.0f, alpha);
  const float q = fminf(fmaxf(om, 1e-10f), 1.0f);
  float Ti = 1.0f;
  {
    float T = 1.0f;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (lane == j) Ti = T;
      T = __fmul_rn(T, lane_bcast(q, j));
    }
  }
  const bool inner = i >= 1 && i <= S - 2;
  const float we = __fadd_rn(__fmul_rn(Ti, alpha), 1e-5f);     // w + eps (used for the inner 62 only)
  const float wsum = torch_sum62_of([&](int k) { return lane_bcast(we, k + 1); });     // bin k <-> lane k + 1; the forward's order
  const float pdf = __fdiv_rn(we, wsum);                       // lane i: pdf of bin i - 1
  float cdf_m = 0.0f;                                          // lane m: cdf[m], m = 0..62
  {
    float run = 0.0f;
#pragma unroll
    for (int m = 1; m < NB; ++m) {
      run = __fadd_rn(run, lane_bcast(pdf, m));
      if (lane == m) cdf_m = run;
    }
  }
  s_cdf[wv][lane] = cdf_m;                                     // (lane 63: unused slot)
  __syncthreads();
  // ---- the two fine samples of this lane: bin, merged slot, adjoint into g_cdf
  const float* gts = g_tsorted + ray * (S + F);
  float* cdf = s_cdf[wv];
  // Everything downstream of the (fp32, forward-identical) decisions is accumulated in float64: the terms num / denom^2 of an
  // ill-conditioned ray (denom ~ 1e-5) are 1e5 x the result of the sums they enter, and the fp32 version of these sums (LDS float
  // atomics + wave scans) was 10-20 x further from a float64 evaluation of the adjoint than torch's fp32 autograd on the same
  // inputs (tests/test_gpu_train_steps.py, round 3).  The kernel is 20 us of a training step either way.
  double* gcdf = s_gcdf[wv];
  int ic_carry = 0;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int k = lane + 64 * half;                             // rank of this fine sample among the ray's (ascending) fine samples
    const float u = RAYS ? us[half] : s_tab[S + k];
    int ind = 0;
    for (int m = 0; m < NB; ++m) ind += cdf[m] <= u;            // cdf is non-decreasing: = the forward's searchsorted(right)
    const int below = min(max(ind - 1, 0), S - 3), above = min(ind, S - 3);
    const float cb = cdf[below], ca = cdf[above];
    const float bb = __fmul_rn(0.5f, __fadd_rn(tc[below + 1], tc[below]));
    const float ba = __fmul_rn(0.5f, __fadd_rn(tc[above + 1], tc[above]));
    const float draw_ = __fsub_rn(ca, cb);
    const bool live = !(draw_ < 1e-5f);
    const float denom = live ? draw_ : 1.0f;
    const float num = __fsub_rn(u, cb);
    const float v = __fadd_rn(bb, __fmul_rn(__fdiv_rn(num, denom), __fsub_rn(ba, bb)));
    int ic = 0;                                                 // coarse entries sorted before this fine sample (ties: coarse first)
    for (int j = 0; j < S; ++j) ic += tc[j] <= v;
    // the forward's merge pointer never moves back: running maximum over the fine samples in order
    ic = max(wave_scan<true>(ic, lane, op_max), ic_carry);
    ic_carry = __shfl(ic, 63);
    const double g = (double)gts[k + ic];                       // its slot in the merged array
    const double g_frac = g * (double)__fsub_rn(ba, bb);
    double g_cb = -g_frac / (double)denom, g_ca = 0.0;          // frac = (u - cb) / denom, denom = ca - cb when live
    if (live) { const double gden = -g_frac * (double)num / ((double)denom * (double)denom); g_ca += gden; g_cb -= gden; }
    atomicAdd(&gcdf[below], g_cb);
    atomicAdd(&gcdf[above], g_ca);
  }
  __syncthreads();
  // ---- cdf[m] = sum_{j<m} pdf_j  ->  g_pdf_j = sum_{m>j} g_cdf[m];  pdf = we / W
  const double sfx = wave_scan<false>(lane < NB ? gcdf[lane] : 0.0, lane, op_sum);
  const double gpdf_excl = wave_shift<false>(sfx, lane, 0.0);   // lane j: g_pdf_j = sum_{m>j} g_cdf[m]
  double gpdf_i = __shfl_up(gpdf_excl, 1);                      // lane i: g_pdf of bin i - 1 (the bin of sample i)
  if (!inner) gpdf_i = 0.0;
  double dot = inner ? gpdf_i * (double)we : 0.0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) dot += __shfl_xor(dot, d);
  const double g_w = inner ? (gpdf_i / (double)wsum - dot / ((double)wsum * (double)wsum)) : 0.0;
  const double sf2 = wave_scan<false>(g_w * (double)alpha * (double)Ti, lane, op_sum);     // suf_i = sum_{m>i} g_w_m a_m T_m
  const double suf = wave_shift<false>(sf2, lane, 0.0);
  double g_alpha = g_w * (double)Ti;
  if (om >= 1e-10f && om <= 1.0f) g_alpha -= suf / (double)q;
  f32x4 go = {0.f, 0.f, 0.f, 0.f};
  go.w = s_raw > 0.0f ? (float)(g_alpha * (double)delta * (double)e) : 0.0f;
  if (ray_ok) reinterpret_cast<f32x4*>(g_raw_c)[ray * S + i] = go;
}

// ------------------------------------------------------------------------------------ stochastic sampling (task == "train")
// Coarse jitter (volume_renderer.py:48-60): mids = 0.5 (t[1:] + t[:-1]), lower = [t0, mids], upper = [mids, t63],
// t = lower + (upper - lower) * jitter, every operation rounded on its own as the CPU torch expression is.
__global__ __launch_bounds__(256)
void nerf_stratified_kernel(const float* __restrict__ t_lin, const float* __restrict__ jitter, long long n, float* __restrict__ t_out) {
  constexpr int S = NERF_N_SAMPLES;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * S) return;
  const int s = (int)(e % S);
  const float lower = s == 0 ? t_lin[0] : __fmul_rn(0.5f, __fadd_rn(t_lin[s], t_lin[s - 1]));
  const float upper = s == S - 1 ? t_lin[S - 1] : __fmul_rn(0.5f, __fadd_rn(t_lin[s + 1], t_lin[s]));
  t_out[e] = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), jitter[e]));
}

// ------------------------------------------------------------------------------------ training: live tiles of a backward pass
// d loss / d raw is exactly zero wherever relu(sigma) = 0 (alpha = 0, weight 0: nerf_composite_bwd_kernel writes zeros there),
// and wherever the coarse density does not move any fine sample.  A 32-point tile (the unit of the chain kernel) whose
// incoming gradient is zero at all its points produces zero g_z rows, adds exactly nothing to any weight gradient and has
// zero g_t / g_x: it is dropped from the chain launch and from every weight-gradient launch.  Exact, not an approximation
// (a zero contribution to a floating-point sum leaves it unchanged); how many tiles are dead is scene-dependent (the
// synthetic bench scene: 23 % of the fine and 36 % of the coarse tiles; a trained scene: most of empty space).
__global__ __launch_bounds__(256)
void nerf_tile_flags_kernel(const f32x4* __restrict__ draw, long long P, int density_only, int* __restrict__ flags) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  bool nz = false;
  if (p < P) {
    const f32x4 g = draw[p];
    nz = density_only ? (g.w != 0.0f) : (g.x != 0.0f || g.y != 0.0f || g.z != 0.0f || g.w != 0.0f);    // (-0 is zero, NaN is not)
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(nz);
  const int lane = threadIdx.x & 63;
  const long long tile = p >> 5;
  if ((lane & 31) == 0 && (p & ~31LL) < P) flags[tile] = (lane ? (b >> 32) : (b & 0xffffffffull)) != 0ull;
}
// flags -> ascending list of live tiles + count; one workgroup (the list is a few thousand entries per pass)
__global__ __launch_bounds__(kScanThreads)
void nerf_tile_scan_kernel(const int* __restrict__ flags, int n_tiles, int* __restrict__ live, int* __restrict__ count) {
  __shared__ int s_cnt[kScanThreads];
  const int total = workgroup_scan(n_tiles, s_cnt, [&](long long t) { return (int)(flags[t] != 0); },
                                   [&](long long t, int pos) { if (flags[t] != 0) live[pos] = (int)t; });
  if (threadIdx.x == 0) *count = total;
}

// ------------------------------------------------------------------------------------ training: the masked (fast_sampling) fine pass
// Ordered stream compaction of the valid (ray, sample) ids: index[0..M) = the ids with valid != 0 in ASCENDING order, *count = M.
// Unlike nerf_compact_kernel (one atomic per wave, arbitrary order: fine for inference, where results are scattered back by id)
// the order here is fixed, because the training forward stores the activations of index[j] at row j of the save buffer: a
// repeatable layout gives repeatable tiles, live-tile lists and gradient sums.  Three launches: per-block counts (256 ids per
// block), one-workgroup exclusive scan of the block counts, ordered scatter.  No atomics.
constexpr int kCompactBlock = kRankBlock;       // compact_block_rank (nerf_scan.hip.inc)
__global__ __launch_bounds__(kCompactBlock)
void nerf_compact_count_kernel(const unsigned char* __restrict__ valid, long long n, int* __restrict__ block_count) {
  __shared__ int s_wave[kCompactBlock / 64];
  const long long i = (long long)blockIdx.x * kCompactBlock + threadIdx.x;
  int total;
  compact_block_rank(i < n && valid[i] != 0, s_wave, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}
// block counts -> exclusive offsets in place, *count = their sum; one workgroup (3072 blocks for a 4096-ray step)
__global__ __launch_bounds__(kScanThreads)
void nerf_compact_scan_kernel(int* __restrict__ block_count, long long n_blocks, int* __restrict__ count) {
  __shared__ int s_cnt[kScanThreads];
  const int total = workgroup_scan(n_blocks, s_cnt, [&](long long b) { return block_count[b]; },
                                   [&](long long b, int pos) { block_count[b] = pos; });
  if (threadIdx.x == 0) *count = total;
}
__global__ __launch_bounds__(kCompactBlock)
void nerf_compact_scatter_kernel(const unsigned char* __restrict__ valid, long long n, const int* __restrict__ block_offset,
                                 int* __restrict__ index) {
  __shared__ int s_wave[kCompactBlock / 64];
  const long long i = (long long)blockIdx.x * kCompactBlock + threadIdx.x;
  const bool v = i < n && valid[i] != 0;
  int total;
  const int rank = compact_block_rank(v, s_wave, total);
  if (v) index[block_offset[blockIdx.x] + rank] = (int)i;       // offset + rank <= number of valid ids before i <= i < n
}

// Masked backward, step 1: the compact rows the chain works on.  Row j < M (= *count) takes d loss / d raw of point index[j]
// and the point itself, x = o + d t with the two roundings of the forward kernels; rows >= M are zero: their tiles are never
// live (nerf_tile_flags_kernel), and the idle rows of the ragged tile behind row M - 1 add exactly nothing.
__global__ __launch_bounds__(256)
void nerf_masked_gather_kernel(const int* __restrict__ index, const int* __restrict__ count, long long P,
                               const f32x4* __restrict__ draw, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                               const float* __restrict__ tvals, long long t_ray_stride, int n_samples,
                               f32x4* __restrict__ draw_c, float* __restrict__ pts_c) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  float x[3] = {0.f, 0.f, 0.f};
  const long long id = j < (long long)*count ? (long long)index[j] : -1;
  if (id >= 0 && id < P) {
    g = draw[id];
    const long long ray = id / n_samples;
    const float t = tvals[ray * t_ray_stride + (id - ray * n_samples)];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(rays_o[ray * 3 + c], __fmul_rn(rays_d[ray * 3 + c], t));
  }
  draw_c[j] = g;
#pragma unroll
  for (int c = 0; c < 3; ++c) pts_c[j * 3 + c] = x[c];
}
// NERF_DEAD_TILE_SKIP=0 with a compact buffer: every tile that holds a listed point is live, whatever its gradient; the tiles
// behind row M - 1 were never written by the forward and stay out.
__global__ __launch_bounds__(256)
void nerf_tile_occupied_kernel(const int* __restrict__ count, long long n_tiles, int* __restrict__ flags) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tiles) flags[t] = t * 32 < (long long)*count;
}
// Masked backward, last step: g_t [P] of the listed points from the chain's compact g_x rows, with the arithmetic of the
// chain's own g_t store (nerf_gt_of_gx_kernel); the caller has zeroed g_t, so unlisted ids keep 0.
__global__ __launch_bounds__(256)
void nerf_masked_gt_scatter_kernel(const int* __restrict__ index, const int* __restrict__ count, long long P,
                                   const float* __restrict__ gx_c, const float* __restrict__ rays_d, int n_samples,
                                   float* __restrict__ g_t) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= P || j >= (long long)*count) return;
  const long long id = index[j];
  if (id < 0 || id >= P) return;
  const long long ray = id / n_samples;
  float gt = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) gt += gx_c[j * 3 + c] * rays_d[ray * 3 + c];
  g_t[id] = gt;
}

// ------------------------------------------------------------------------------------ fused clip + Adam (section 8f-4)
// One launch over all 48 parameter tensors: clip_grad_value_ (trainer.py:59) + torch.optim.Adam's update
// (optimizer.py:21-24: Adam(lr, weight_decay, eps), betas (0.9, 0.999), no amsgrad) in torch's operation
// order (lerp for exp_avg, sqrt(v)/sqrt(bc2) + eps for the denominator).
constexpr int kAdamMaxTensors = 48;
struct AdamArgs {
  float* p[kAdamMaxTensors];
  const float* g[kAdamMaxTensors];
  float* m[kAdamMaxTensors];
  float* v[kAdamMaxTensors];
  long long end[kAdamMaxTensors];      // exclusive prefix ends of the flattened index space
  int n_tensors;
  float lr, beta1, beta2, eps, weight_decay, clip, bc1, bc2_sqrt;
};
__global__ __launch_bounds__(256)
void nerf_adam_kernel(AdamArgs a) {
  const long long total = a.end[a.n_tensors - 1];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = a.n_tensors - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (i < a.end[mid]) hi = mid; else lo = mid + 1; }
    const long long j = i - (lo ? a.end[lo - 1] : 0);
    float g = a.g[lo][j];
    if (a.clip > 0.0f) g = fminf(fmaxf(g, -a.clip), a.clip);
    const float p = a.p[lo][j];
    if (a.weight_decay != 0.0f) g = __fadd_rn(g, __fmul_rn(a.weight_decay, p));
    float m = a.m[lo][j], v = a.v[lo][j];
    m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), 1.0f - a.beta1));                       // exp_avg.lerp_(grad, 1 - beta1)
    v = __fadd_rn(__fmul_rn(v, a.beta2), __fmul_rn(__fmul_rn(g, g), 1.0f - a.beta2));   // mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt), a.eps);
    a.m[lo][j] = m; a.v[lo][j] = v;
    a.p[lo][j] = __fadd_rn(p, __fmul_rn(-(a.lr / a.bc1), __fdiv_rn(m, denom)));         // addcdiv_(m, denom, value=-step_size)
  }
}

// ------------------------------------------------------------------------------------ ray generation
// Pinhole rays of src/datasets/nerf/blender.py:102-127 in float64 like numpy, cast to float32 at the
// end (:149-151).  One thread per pixel; removes the 15.4 MB/frame host->device copy of run.py:167-169.
struct RayGenArgs {
  double c2w[12];          // row-major 3x4 camera-to-world
  double focal, cx, cy;
  long long pixel_begin, n_pixels;
  int W;
  const long long* pixel_ids;   // optional explicit pixel list (training batches), else pixel_begin + i
  float* rays_o;
  float* rays_d;
};
__global__ void nerf_generate_rays_kernel(RayGenArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_pixels) return;
  const long long id = a.pixel_ids ? a.pixel_ids[i] : a.pixel_begin + i;
  const double u = (double)(id % a.W), v = (double)(id / a.W);
  const double dx = (u - a.cx) / a.focal, dy = -(v - a.cy) / a.focal, dz = -1.0;
  double w[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = (a.c2w[4 * r + 0] * dx + a.c2w[4 * r + 1] * dy) + a.c2w[4 * r + 2] * dz;
  const double nrm = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    a.rays_d[i * 3 + r] = (float)(w[r] / nrm);
    a.rays_o[i * 3 + r] = (float)a.c2w[4 * r + 3];
  }
}

// ------------------------------------------------------------------------------------ image metrics
// Sums for src/evaluators/nerf.py: float MSE of the clipped images (:96-100) and the evaluator's
// psnr_metric (:23-30), whose uint8 subtraction AND squaring wrap modulo 256.
__global__ __launch_bounds__(256)
void nerf_image_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long long n_values,
                               double* __restrict__ out /*[2]: sum sq float, sum wrapped-u8 sq*/) {
  double s_f = 0.0, s_u = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_values; i += (long long)gridDim.x * blockDim.x) {
    const float p = fminf(fmaxf(pred[i], 0.0f), 1.0f), g = fminf(fmaxf(gt[i], 0.0f), 1.0f);
    const float d = p - g;
    s_f += (double)(d * d);
    const unsigned pu = (unsigned)(p * 255.0f) & 0xffu, gu = (unsigned)(g * 255.0f) & 0xffu;   // astype(uint8): truncation
    const unsigned du = (pu - gu) & 0xffu;
    s_u += (double)((du * du) & 0xffu);
  }
  __shared__ double red[2][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s_f += __shfl_xor(s_f, o); s_u += __shfl_xor(s_u, o); }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = s_f; red[1][wave] = s_u; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&out[0], (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    atomicAdd(&out[1], (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
  }
}

// SSIM of src/evaluators/nerf.py:49-77: skimage.metrics.structural_similarity(pred_u8, gt_u8, win_size=7,
// channel_axis=2) = Wang et al. with a 7x7 uniform window, sample covariance (49/48), K1 .01, K2 .03,
// data_range 255, mean over the (H-6)x(W-6) interior and the 3 channels; float64 like skimage.
__global__ __launch_bounds__(256)
void nerf_ssim_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W, double* __restrict__ out) {
  const long long n_int = (long long)(H - 6) * (W - 6) * 3;
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_int; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % 3);
    const long long px = i / 3;
    const int x = (int)(px % (W - 6)) + 3, y = (int)(px / (W - 6)) + 3;
    double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int dy = -3; dy <= 3; ++dy)
      for (int dx = -3; dx <= 3; ++dx) {
        const long long q = ((long long)(y + dy) * W + (x + dx)) * 3 + c;
        const double a = (double)((unsigned)(fminf(fmaxf(pred[q], 0.f), 1.f) * 255.0f) & 0xffu);
        const double b = (double)((unsigned)(fminf(fmaxf(gt[q], 0.f), 1.f) * 255.0f) & 0xffu);
        sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
      }
    const double ux = sx / 49.0, uy = sy / 49.0, cn = 49.0 / 48.0;
    const double vx = cn * (sxx / 49.0 - ux * ux), vy = cn * (syy / 49.0 - uy * uy), vxy = cn * (sxy / 49.0 - ux * uy);
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    s += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}

// ------------------------------------------------------------------------------------ d loss / d viewdirs (Network.forward under autograd)
// The view direction of a ray enters views_linears.0 through its 27-channel encoding (network.py:224-225, :63-66) and is
// shared by the ray's samples: g_dir_enc = W_v[:, 256:283]^T (sum_s g_zv[ray, s]), then the chain rule through
// [d, sin(2^k d), cos(2^k d)] (freq.py:31-32).  One 128-thread workgroup per ray; 3.5 k MACs per ray -- negligible.
// viewdir_grad_block: the part after the sum, shared by the point-mode and the ray-mode entry.  Thread o brings column o of
// sum_s g_zv (`acc`) and, for o < 3, component o of the direction the forward encoded (`dir`); threads 0..2 get component o
// of d loss / d dir back.
__device__ __forceinline__ float viewdir_grad_block(float acc, float dir, const float* __restrict__ w_views, float* G, float* E) {
  const int o = threadIdx.x;
  G[o] = acc;
  __syncthreads();
  if (o < 27) {
    float e = 0.0f;
    for (int k = 0; k < 128; ++k) e = fmaf(G[k], w_views[k * 283 + 256 + o], e);
    E[o] = e;
  }
  __syncthreads();
  float g = 0.0f;
  if (o < 3) {
    g = E[o];
    for (int k = 0; k < 4; ++k) {
      const float f = (float)(1 << k);
      float sv, cv;
      sincosf(dir * f, &sv, &cv);
      g += f * (cv * E[3 + 6 * k + o] - sv * E[3 + 6 * k + 3 + o]);
    }
  }
  return g;
}

__global__ __launch_bounds__(128)
void nerf_viewdirs_bwd_kernel(const float* __restrict__ gzv, long long n_rays, int n_samples, const float* __restrict__ w_views,
                              const float* __restrict__ viewdirs, float* __restrict__ g_viewdirs) {
  __shared__ float G[128];
  __shared__ float E[27];
  const long long ray = blockIdx.x;
  const int o = threadIdx.x;
  float acc = 0.0f;
  for (int s = 0; s < n_samples; ++s) acc += gzv[(ray * n_samples + s) * 128 + o];
  const float g = viewdir_grad_block(acc, o < 3 ? viewdirs[ray * 3 + o] : 0.0f, w_views, G, E);
  if (o < 3) g_viewdirs[ray * 3 + o] = g;
}

// ------------------------------------------------------------------------------------ d loss / d rays (Renderer.render under autograd)
// The rays adjoint ("Gradients with respect to the rays").  Ray mode: the fine pass encodes v = d / |d|, rounded
// as the forward kernels do, so g_d gets J_norm(d)^T g_v = (g_v - v (v . g_v)) / |d| from the fine pass's g_zv rows.  A dead tile
// (flag 0 in the list of the pass, TrainGrad::off_flags) has no workgroup and unwritten g_zv rows: it is skipped here, exactly (its
// rows would be zero).  Without a list (*count == -1) every row was written.
__global__ __launch_bounds__(128)
void nerf_rays_viewdirs_bwd_kernel(const float* __restrict__ gzv, const int* __restrict__ flags, const int* __restrict__ count,
                                   int n_samples, const float* __restrict__ w_views, const float* __restrict__ rays_d,
                                   float* __restrict__ g_dview) {
  __shared__ float G[128];
  __shared__ float E[27];
  const long long ray = blockIdx.x;
  const int o = threadIdx.x;
  const bool list = *count >= 0;
  float acc = 0.0f;
  for (int s = 0; s < n_samples; ++s) {
    const long long p = ray * n_samples + s;
    if (list && flags[p >> 5] == 0) continue;          // (uniform)
    acc += gzv[p * 128 + o];
  }
  float nrm = 1.0f, v = 0.0f;
  if (o < 3) {
    const float d0 = rays_d[ray * 3 + 0], d1 = rays_d[ray * 3 + 1], d2 = rays_d[ray * 3 + 2];
    nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
    v = __fdiv_rn(o == 0 ? d0 : o == 1 ? d1 : d2, nrm);
  }
  const float gv = viewdir_grad_block(acc, v, w_views, G, E);
  const float vg = __shfl(v, 0) * __shfl(gv, 0) + __shfl(v, 1) * __shfl(gv, 1) + __shfl(v, 2) * __shfl(gv, 2);
  if (o < 3) g_dview[ray * 3 + o] = (gv - v * vg) / nrm;
}

// g_t [P] = g_x . d of the point's ray, after a chain that wrote g_x (BwdArgs::g_t bit 0): the arithmetic of the chain's own
// g_t store (gt = 0; gt += g_x[c] * d[c], c = 0..2), so the result is bit-identical to a call without g_x.
__global__ __launch_bounds__(256)
void nerf_gt_of_gx_kernel(const float* __restrict__ gx, const float* __restrict__ rays_d, int n_samples, long long P,
                          float* __restrict__ g_t) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long long ray = p / n_samples;
  float gt = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) gt += gx[p * 3 + c] * rays_d[ray * 3 + c];
  g_t[p] = gt;
}

// Per-ray sums of the rays adjoint: x = o + d t at the 64 coarse and the 192 merged fine samples, so
//   g_o = sum_s gx_c + sum_s gx_f,   g_d = sum_s t_c gx_c + sum_s t_s gx_f + g_dview.
// One wave per ray: lane l takes coarse sample l and fine samples l, l + 64, l + 128; a fixed xor butterfly finishes the sums
// (no atomics: the result does not depend on scheduling).  gx_c / gx_f / g_dview may each be null (term left out).
__global__ __launch_bounds__(256)
void nerf_rays_bwd_kernel(long long n_rays, const float* __restrict__ t_c, long long t_stride, const float* __restrict__ gx_c,
                          const float* __restrict__ t_s, const float* __restrict__ gx_f, const float* __restrict__ g_dview,
                          float* __restrict__ g_o, float* __restrict__ g_d) {
  constexpr int S_C = NERF_N_SAMPLES, S_F = NERF_N_SAMPLES + NERF_N_IMPORTANCE;
  static_assert(S_C == 64 && S_F % 64 == 0, "one coarse sample per lane");
  const int lane = threadIdx.x & 63;
  const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;                           // (whole waves; no barrier below)
  float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
  if (gx_c != nullptr) {
    const float t = t_c[ray * t_stride + lane];
    const long long p = ray * S_C + lane;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float g = gx_c[p * 3 + c];
      so[c] += g; sd[c] += t * g;
    }
  }
  if (gx_f != nullptr) {
#pragma unroll
    for (int k = 0; k < S_F / 64; ++k) {
      const long long p = ray * S_F + k * 64 + lane;
      const float t = t_s[p];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float g = gx_f[p * 3 + c];
        so[c] += g; sd[c] += t * g;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int c = 0; c < 3; ++c) { so[c] += __shfl_xor(so[c], off); sd[c] += __shfl_xor(sd[c], off); }
  if (lane < 3) {
    const float o_l = lane == 0 ? so[0] : lane == 1 ? so[1] : so[2];
    const float d_l = lane == 0 ? sd[0] : lane == 1 ? sd[1] : sd[2];
    g_o[ray * 3 + lane] = o_l;
    g_d[ray * 3 + lane] = g_dview != nullptr ? d_l + g_dview[ray * 3 + lane] : d_l;
  }
}

// ------------------------------------------------------------------------------------ dead-tile skipping: ONE decision for both passes
// The SAVE forward for compositing drops the rows of density-free tiles, and the backward pass drops tiles without an incoming
// gradient: the second is only safe to switch off if the first was off too (a dense backward would read rows that were never
// written).  Both entry points therefore ask this one helper, and the forward stamps what it did into the save buffer
// (TrainSave::off_stamp): a dense backward on a buffer stamped "rows skipped" poisons the alpha-bias gradient with NaN instead
// of silently multiplying garbage by zero (the host cannot read the stamp without a synchronisation the ABI does not make).
bool dead_tile_list_available(long long P, int precision) {
  const char* env = getenv("NERF_DEAD_TILE_SKIP");
  const bool want = !(env && env[0] == '0');
  return want && (precision == NERF_PREC_F32 || precision == NERF_PREC_F32X) && P % 32 == 0 && P / 32 <= 0x7fffffffLL;
}
__global__ void nerf_check_stamp_kernel(const float* __restrict__ stamp, float* __restrict__ poison) {
  if (threadIdx.x == 0 && __float_as_int(stamp[0]) != 0) poison[0] = __int_as_float(0x7fc00000);
}

// ------------------------------------------------------------------------------------ launch helpers
int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    cus = v;
  }
  return cus;
}

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Every workspace is ONE layout struct that takes its pieces from a Carver, in order, each 256-byte aligned: built on the
// caller's pointer it holds the pieces, built on a null base its bytes() is what the *_workspace_bytes entry reports.
struct Carver {
  uintptr_t base, p;
  explicit Carver(const void* b) : base((uintptr_t)b), p((uintptr_t)b) {}
  template <class T> T* take(int64_t count) {
    T* q = (T*)p;
    p += (uintptr_t)align256(count * (int64_t)sizeof(T));
    return q;
  }
  int64_t bytes() const { return (int64_t)(p - base); }
};

}  // namespace

// ===================================================================================== C ABI
extern "C" {

// The MLP forward instances of one precision, inference or SAVE (training forward), and their launch shape.
using MlpKernel = void (*)(MlpArgs);
struct MlpFamily {
  const char* name;
  int wg_pts, threads;       // points and threads of one workgroup tile
  bool persistent;           // one workgroup per CU walks the tiles; otherwise one workgroup per tile
  MlpKernel inst[4];         // rays, density only | rays, dead-colour skip | rays | points
};
#define NERF_MLP_INFERENCE_3(K) {K<true, true>, K<true, false, true>, K<true>, K<false>}
#define NERF_MLP_INFERENCE_4(K) {K<true, false, true>, K<true, false, false, true>, K<true>, K<false>}
#define NERF_MLP_SAVE(K) {K<true, true, true>, K<true, true, false, true>, K<true, true>, K<false, true>}
static const MlpFamily kMlpF32x = {"nerf_mlp_f32x_kernel", kXTilePts, kXThreads, true, NERF_MLP_INFERENCE_4(nerf_mlp_f32x_kernel)};
// the fp16 path on 16x16x32 MFMA tiles: same workgroup shape and LDS ring as f16 (147 KB of LDS per workgroup)
static const MlpFamily kMlpF16s = {"nerf_mlp_f16s_kernel", kF16TilePts, kF16Threads, true, NERF_MLP_INFERENCE_3(nerf_mlp_f16s_kernel)};
static const MlpFamily kMlpF16 = {"nerf_mlp_f16_kernel", kF16TilePts, kF16Threads, true, NERF_MLP_INFERENCE_3(nerf_mlp_f16_kernel)};
// barrier-free: workgroups of NERF_F32_WG_WAVES one-tile waves (nerf_mlp_f32.hip.inc says why one)
static const MlpFamily kMlpF32 = {"nerf_mlp_f32_kernel", nerf::kTilePts * NERF_F32_WG_WAVES, 64 * NERF_F32_WG_WAVES, false,
                           NERF_MLP_INFERENCE_4(nerf_mlp_f32_kernel)};
// the SAVE families (training forward): one-wave workgroups for f32
static const MlpFamily kMlpSaveF32x = {"nerf_mlp_f32x_kernel", kXTilePts, kXThreads, true, NERF_MLP_SAVE(nerf_mlp_f32x_kernel)};
static const MlpFamily kMlpSaveF32 = {"nerf_mlp_f32_kernel", nerf::kTilePts, 64, false, NERF_MLP_SAVE(nerf_mlp_f32_kernel)};
static const MlpFamily* mlp_family(int precision, bool save) {
  switch (precision) {
    case NERF_PREC_F32: return save ? &kMlpSaveF32 : &kMlpF32;
    case NERF_PREC_F32X: return save ? &kMlpSaveF32x : &kMlpF32x;
    case NERF_PREC_F16: return save ? nullptr : &kMlpF16;
    case NERF_PREC_F16S: return save ? nullptr : &kMlpF16s;
  }
  return nullptr;
}

// persistent kernels: one workgroup per CU, fewer when there are fewer tiles
static unsigned persistent_blocks(long long n_points, int wg_pts) {
  const long long n_tiles = (n_points + wg_pts - 1) / wg_pts;
  return (unsigned)(n_tiles < num_cus() ? n_tiles : num_cus());
}

// every MLP forward launch: the family from (precision, save), the instance from (ray_mode, density_only, skip_dead_colour).
// `entry`: the public function that was called (error texts)
static int launch_mlp(const MlpArgs& a_in, bool ray_mode, bool save, int precision, hipStream_t st, const char* entry) {
  if (!mlp_family(precision, false)) return fail(NERF_ERR_UNSUPPORTED, "%s: precision not built", entry);
  if (a_in.n_points <= 0) return NERF_OK;
  MlpArgs a = a_in;
  if (a.index && a.n_points > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s: index mode: point ids are int32", entry);
  const MlpFamily* f = mlp_family(precision, save);
  if (!f) return fail(NERF_ERR_UNSUPPORTED, "%s: f32 or f32x only", entry);
  // density_only (ray mode): every precision has an instance that stops after the sigma head
  const MlpKernel k = f->inst[!ray_mode ? 3 : a.density_only ? 0 : a.skip_dead_colour ? 1 : 2];
  if (precision == NERF_PREC_F32) a.fold = a.packed + nerf::kOffFold;
  if (f->persistent) return launch(f->name, k, dim3(persistent_blocks(a.n_points, f->wg_pts)), dim3(f->threads), st, a);
  const long long blocks = (a.n_points + f->wg_pts - 1) / f->wg_pts;
  if (blocks > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s: too many points for one launch", entry);
  return launch(f->name, k, dim3((unsigned)blocks), dim3(f->threads), st, a);
}

// The ray-mode forward entries.  for_compositing: `raw` only ever reaches nerf_composite, where the colours of zero-density
// samples are multiplied by exactly 0, so tiles without density skip the colour branch (DSKIP).  want_save: the training forward.
// index / count (masked): rows of index[j] at slot j, `raw` at the id (every instance honours both).
static int forward_rays(const char* entry, const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                        int32_t n_samples, const void* packed, float* raw, bool want_save, float* save, bool density_only,
                        bool for_compositing, int32_t precision, void* stream, const int* index = nullptr, const int* count = nullptr) {
  if (n_rays < 0 || n_samples <= 0 || t_ray_stride < 0) return fail(NERF_ERR_INVALID_ARG, "%s: bad size", entry);
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !tvals || !packed || !raw || (want_save && !save)) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  MlpArgs a{};
  a.rays_o = rays_o; a.rays_d = rays_d; a.tvals = tvals; a.t_ray_stride = t_ray_stride;
  a.n_points = n_rays * n_samples; a.n_samples = n_samples; a.packed = (const float*)packed; a.raw = raw; a.save = save;
  a.density_only = density_only; a.skip_dead_colour = for_compositing;
  a.index = index; a.count = count;
  if (want_save) {
    // without dead-tile skipping in the backward pass every row must exist: fall back to the full store (the SAME helper decides
    // for the backward pass).  The buffer is stamped with what is done here: 1 = the rows of density-free tiles are NOT stored
    a.skip_dead_colour = for_compositing && dead_tile_list_available(a.n_points, precision);
    if (hipMemsetAsync(save + TrainSave::off_stamp(a.n_points), a.skip_dead_colour ? 0x01 : 0x00, 4 * sizeof(float), (hipStream_t)stream) != hipSuccess)
      return fail(NERF_ERR_HIP, "%s: memset failed", entry);
  }
  return launch_mlp(a, true, want_save, precision, (hipStream_t)stream, entry);
}

int32_t nerf_abi_version(void) { return NERF_ABI_VERSION; }

int32_t nerf_build_flags(void) {
  int32_t f = 0;
#ifdef NERF_TIMING_BUILD
  f |= NERF_BUILD_TIMING;
#endif
#if NERF_ANY_TIMING_HACK || NERF_SAVE_TAPS == 0
  f |= NERF_BUILD_WRONG_NUMERICS;
#endif
  return f;
}
const char* nerf_last_error(void) { return g_err; }
int64_t nerf_packed_model_bytes(int32_t precision) {
  if (precision == NERF_PREC_F32) return nerf::kPackedFloats * (int64_t)sizeof(float);
  // the fp16 streams carry the split-fp16 ("f32x") stream of the same model behind them: nerf_render_forward re-evaluates the
  // last sample of every ray with it (far-plane guard)
  if (precision == NERF_PREC_F16 || precision == NERF_PREC_F16S) return nerf::kF16PackedBytes + nerf::kXPackedBytes;
  if (precision == NERF_PREC_F32X) return nerf::kXPackedBytes;
  return -1;
}

// the PackArgs of every pack entry (`entry`: its name for the error text)
static int32_t fill_pack_args(const char* entry, const float* const params[24], void* out, PackArgs& a) {
  if (!params || !out) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  for (int i = 0; i < nerf::P_COUNT; ++i) {
    if (!params[i]) return fail(NERF_ERR_INVALID_ARG, "%s: null parameter pointer", entry);
    a.p[i] = params[i];
  }
  a.out = (float*)out;
  return NERF_OK;
}

int32_t nerf_pack_model(const float* const params[24], void* packed, int32_t precision, void* stream) {
  PackArgs a;
  if (const int rc = fill_pack_args("nerf_pack_model", params, packed, a)) return rc;
  const int threads = 256;
  if (precision == NERF_PREC_F16 || precision == NERF_PREC_F32X || precision == NERF_PREC_F16S) {
    const long long n = nerf::kF16ConstBytes / 4 + (long long)nerf::kF16Frags * 512;
    const dim3 grid((unsigned)((n + threads - 1) / threads));
    hipStream_t st = (hipStream_t)stream;
    if (precision == NERF_PREC_F32X) return NERF_LAUNCH(nerf_pack_f16_kernel<true>, grid, dim3(threads), st, a);
    if (const int rc = precision == NERF_PREC_F16S ? NERF_LAUNCH(nerf_pack_f16s_kernel, grid, dim3(threads), st, a)
                                                   : NERF_LAUNCH(nerf_pack_f16_kernel<false>, grid, dim3(threads), st, a))
      return rc;
    PackArgs ax = a;                            // + the f32x stream behind the fp16 one
    ax.out = reinterpret_cast<float*>(reinterpret_cast<char*>(packed) + nerf::kF16PackedBytes);
    return NERF_LAUNCH(nerf_pack_f16_kernel<true>, grid, dim3(threads), st, ax);
  }
  if (precision != NERF_PREC_F32) return fail(NERF_ERR_UNSUPPORTED, "%s", "nerf_pack_model: unknown precision");
  const unsigned blocks = (unsigned)((nerf::kUnfoldedFloats + threads - 1) / threads);
  if (const int rc = NERF_LAUNCH(nerf_pack_kernel, dim3(blocks), dim3(threads), (hipStream_t)stream, a)) return rc;
  return NERF_LAUNCH(nerf_fold_f32_kernel, dim3(kFoldBlocks), dim3(256), (hipStream_t)stream, (const float*)a.out, a.out + nerf::kOffFold);
}

int32_t nerf_positional_encoding(const float* x, int64_t n, int32_t n_freqs, float* out, void* stream) {
  if (n < 0 || n_freqs < 0 || n_freqs > 16) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_positional_encoding: bad size");
  if (n == 0) return NERF_OK;
  if (!x || !out) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_positional_encoding: null argument");
  const unsigned blocks = (unsigned)((n * 3 + 255) / 256);
  return NERF_LAUNCH(nerf_pe_kernel, dim3(blocks), dim3(256), (hipStream_t)stream, x, (long long)n, n_freqs, out);
}

int32_t nerf_mlp_forward(const float* pts, const float* viewdirs, int64_t n_rays, int32_t n_samples,
                         const void* packed, float* raw, int32_t precision, void* stream) {
  if (n_rays < 0 || n_samples <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_forward: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!pts || !viewdirs || !packed || !raw) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_forward: null argument");
  MlpArgs a{};
  a.pts = pts; a.viewdirs = viewdirs; a.n_points = n_rays * n_samples; a.n_samples = n_samples;
  a.packed = (const float*)packed; a.raw = raw;
  return launch_mlp(a, false, false, precision, (hipStream_t)stream, "nerf_mlp_forward");
}

int32_t nerf_mlp_forward_rays(const float* rays_o, const float* rays_d, const float* tvals,
                              int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                              const void* packed, float* raw, int32_t precision, void* stream) {
  return forward_rays("nerf_mlp_forward_rays", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed, raw, false, nullptr,
                      false, false, precision, stream);
}

int32_t nerf_mlp_forward_rays_for_compositing(const float* rays_o, const float* rays_d, const float* tvals,
                                              int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                              const void* packed, float* raw, int32_t precision, void* stream) {
  return forward_rays("nerf_mlp_forward_rays_for_compositing", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed, raw,
                      false, nullptr, false, true, precision, stream);
}

int32_t nerf_mlp_forward_rays_density(const float* rays_o, const float* rays_d, const float* tvals,
                                      int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                      const void* packed, float* raw, int32_t precision, void* stream) {
  return forward_rays("nerf_mlp_forward_rays_density", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed, raw, false,
                      nullptr, true, false, precision, stream);
}

static bool bad_strides(int64_t t_ray_stride, int64_t u_ray_stride) {
  return (t_ray_stride != 0 && t_ray_stride != NERF_N_SAMPLES) || (u_ray_stride != 0 && u_ray_stride != NERF_N_IMPORTANCE);
}
// nerf_sample_fine (shared tables: both strides 0) and nerf_sample_fine_rays behind their own size checks.  Shared tables take
// the <false> instance, a table per ray of either kind the <true> one.
static int32_t sample_fine(const char* entry, const float* raw_coarse, const float* t_coarse, int64_t t_ray_stride, const float* u,
                           int64_t u_ray_stride, int64_t n_rays, float* t_sorted, float* t_fine, uint8_t* valid_sorted,
                           float weights_threshold, float ert_threshold, void* stream) {
  const bool per_ray = t_ray_stride != 0 || u_ray_stride != 0;
  if (per_ray && valid_sorted) return fail(NERF_ERR_INVALID_ARG, "%s: fast_sampling needs the shared tables", entry);
  if (n_rays == 0) return NERF_OK;
  if (!raw_coarse || !t_coarse || !u || !t_sorted) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  SampleArgs a;
  a.raw_c = raw_coarse; a.t_coarse = t_coarse; a.t_stride = t_ray_stride; a.u = u; a.u_stride = u_ray_stride; a.n_rays = n_rays;
  a.t_sorted = t_sorted; a.t_fine = t_fine; a.valid_sorted = valid_sorted; a.fast_sampling = valid_sorted != nullptr;
  a.weights_threshold = per_ray ? 0.0f : weights_threshold; a.ert_threshold = per_ray ? 0.0f : ert_threshold;
  const dim3 blocks((unsigned)((n_rays + kSampleThreads - 1) / kSampleThreads));
  return per_ray ? NERF_LAUNCH(nerf_sample_fine_kernel<true>, blocks, dim3(kSampleThreads), (hipStream_t)stream, a)
                 : NERF_LAUNCH(nerf_sample_fine_kernel<false>, blocks, dim3(kSampleThreads), (hipStream_t)stream, a);
}
int32_t nerf_sample_fine(const float* raw_coarse, const float* t_coarse, const float* u,
                         int64_t n_rays, float* t_sorted, float* t_fine, uint8_t* valid_sorted,
                         float weights_threshold, float ert_threshold, void* stream) {
  if (n_rays < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sample_fine: bad size");
  return sample_fine("nerf_sample_fine", raw_coarse, t_coarse, 0, u, 0, n_rays, t_sorted, t_fine, valid_sorted, weights_threshold,
                     ert_threshold, stream);
}
int32_t nerf_sample_fine_rays(const float* raw_coarse, const float* t_coarse, int64_t t_ray_stride, const float* u,
                              int64_t u_ray_stride, int64_t n_rays, float* t_sorted, float* t_fine, uint8_t* valid_sorted,
                              float weights_threshold, float ert_threshold, void* stream) {
  if (n_rays < 0 || bad_strides(t_ray_stride, u_ray_stride))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sample_fine_rays: bad size or stride (t: 0 or 64, u: 0 or 128)");
  return sample_fine("nerf_sample_fine_rays", raw_coarse, t_coarse, t_ray_stride, u, u_ray_stride, n_rays, t_sorted, t_fine, valid_sorted,
                     weights_threshold, ert_threshold, stream);
}

int32_t nerf_composite(const float* raw, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                       int32_t n_samples, int32_t white_bkgd, float* rgb, float* depth,
                       float* weights, void* stream) {
  if (n_rays < 0 || n_samples <= 0 || t_ray_stride < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!raw || !tvals || !rgb || !depth) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite: null argument");
  if (n_samples % kCompChunk == 0 && (t_ray_stride % 4 == 0) && ((uintptr_t)tvals % 16 == 0)) {
    return NERF_LAUNCH(nerf_composite_staged_kernel, dim3((unsigned)((n_rays + 63) / 64)), dim3(64), (hipStream_t)stream, raw, tvals,
                       (long long)t_ray_stride, (long long)n_rays, n_samples, white_bkgd, rgb, depth, weights);
  }
  const unsigned blocks = (unsigned)((n_rays + 255) / 256);
  return NERF_LAUNCH(nerf_composite_kernel, dim3(blocks), dim3(256), (hipStream_t)stream, raw, tvals, (long long)t_ray_stride,
                     (long long)n_rays, n_samples, white_bkgd, rgb, depth, weights);
}

int32_t nerf_generate_rays(const double c2w[12], int32_t H, int32_t W, double focal, int64_t pixel_begin,
                           int64_t n_pixels, const int64_t* pixel_ids, float* rays_o, float* rays_d, void* stream) {
  if (n_pixels < 0 || H <= 0 || W <= 0 || !(focal > 0.0) || pixel_begin < 0 ||
      (!pixel_ids && pixel_begin + n_pixels > (int64_t)H * W))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_generate_rays: bad size");
  if (n_pixels == 0) return NERF_OK;
  if (!c2w || !rays_o || !rays_d) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_generate_rays: null argument");
  RayGenArgs a;
  for (int i = 0; i < 12; ++i) a.c2w[i] = c2w[i];
  a.focal = focal; a.cx = W / 2.0; a.cy = H / 2.0; a.pixel_begin = pixel_begin; a.n_pixels = n_pixels; a.W = W;
  a.pixel_ids = (const long long*)pixel_ids; a.rays_o = rays_o; a.rays_d = rays_d;
  return NERF_LAUNCH(nerf_generate_rays_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), (hipStream_t)stream, a);
}

int32_t nerf_image_metrics(const float* pred, const float* gt, int64_t n_values, double* sums2, void* stream) {
  if (n_values < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_image_metrics: bad size");
  if (!sums2) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_image_metrics: null argument");
  if (hipMemsetAsync(sums2, 0, 2 * sizeof(double), (hipStream_t)stream) != hipSuccess)
    return fail(NERF_ERR_HIP, "%s", "nerf_image_metrics: memset failed");
  if (n_values == 0) return NERF_OK;
  if (!pred || !gt) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_image_metrics: null argument");
  long long blocks = (n_values + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  return NERF_LAUNCH(nerf_image_metrics_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, pred, gt, (long long)n_values,
                     sums2);
}

// The 256 x 256 layers on the operand ring, 1..8 of them in one launch of `slices` workgroups per job.  The caller has checked the
// ring's host contract (nerf_wgrad_f32.hip.inc): aligned 256 x 256 jobs of n_points % 16 == 0 points with ld * 8 < 2^31
static int32_t wgrad256_ring(WgradBatch& wb, long long slices, const int* live, const int* n_live, hipStream_t st) {
  for (int i = 0; i < wb.n_jobs; ++i) {
    WgradArgs& j = wb.job[i];
    j.n_out = 256; j.n_in = 256; j.osplit = 2; j.isplit = 2; j.live_tiles = live; j.n_live = n_live;
  }
  const dim3 grid((unsigned)(slices * wb.n_jobs)), blk(256);
  return live ? NERF_LAUNCH(nerf_wgrad256_f32_asm_kernel<true>, grid, blk, st, wb)
              : NERF_LAUNCH(nerf_wgrad256_f32_asm_kernel<false>, grid, blk, st, wb);
}

// Row R of nerf::kWgRows in the form wg_choose picked: the kernels are instantiated from the table's own numbers.  With a list
// every CU's workgroup reads *n_live itself; without one the ring form takes one workgroup per group of 16 k-steps, at most one
// per CU; the plain forms take `grid` (one workgroup per CU too: more resident waves measured no faster)
extern "C++" {
template <int R>
static int32_t wgrad_launch_row(nerf::WgForm form, WgradArgs& a, dim3 grid, hipStream_t st) {
  constexpr nerf::WgRow r = nerf::kWgRows[R];
  const dim3 blk(256);
  a.osplit = r.osplit; a.isplit = r.isplit;
  if constexpr (r.kind == nerf::kWgVecRing) {
    const long long groups = a.n_points / 32;
    if (form == nerf::kWgList) return NERF_LAUNCH((nerf_wgrad_vec_f32_asm_kernel<r.wo, r.wi, 16, true>), dim3((unsigned)num_cus()), blk, st, a);
    if (form == nerf::kWgRing) return NERF_LAUNCH((nerf_wgrad_vec_f32_asm_kernel<r.wo, r.wi, 16>), dim3((unsigned)(groups < num_cus() ? groups : num_cus())), blk, st, a);
  }
  if constexpr (r.kind == nerf::kWgGeneric) return NERF_LAUNCH((nerf_wgrad_f32_kernel<r.wo, r.wi>), grid, blk, st, a);
  else return NERF_LAUNCH((nerf_wgrad_vec_f32_kernel<r.wo, r.wi>), grid, blk, st, a);
}
template <int... R>
static int32_t wgrad_launch(nerf::WgChoice c, WgradArgs& a, dim3 grid, hipStream_t st, std::integer_sequence<int, R...>) {
  int32_t rc = NERF_ERR_INVALID_ARG;
  (void)((c.row == R && ((rc = wgrad_launch_row<R>(c.form, a, grid, st)), true)) || ...);
  return rc;
}
}  // extern "C++"

// live / n_live: the live-tile list of a backward pass (device pointers) or nullptr for the whole point range; with a list,
// only the asm-ring kernels of the small layers apply (the caller checks list_mode_ok) and each workgroup reads *n_live itself
static int32_t wgrad_impl(const float* dz, int64_t ldz, int32_t zc0, int32_t n_out, const float* hin, int64_t ldh,
                          int32_t hc0, int32_t n_in, float* dw, int64_t ldw, int32_t wc0, float* db, int64_t n_points,
                          const int* live, const int* n_live, void* stream) {
  if (n_points < 0 || n_out <= 0 || n_in <= 0 || n_out > 256 || n_in > 256) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_wgrad: bad size");
  if (n_points == 0) return NERF_OK;
  if (!dz || !hin || !dw) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_wgrad: null argument");
  WgradArgs a;
  a.dz = dz; a.ldz = ldz; a.zc0 = zc0; a.n_out = n_out; a.hin = hin; a.ldh = ldh; a.hc0 = hc0; a.n_in = n_in;
  a.dw = dw; a.ldw = ldw; a.wc0 = wc0; a.db = db; a.n_points = n_points; a.live_tiles = live; a.n_live = n_live;
  const long long pairs = (n_points + 1) / 2;
  long long blocks = (pairs + 255) / 256;            // >= 256 point pairs per workgroup
  if (blocks > num_cus()) blocks = num_cus();
  if (blocks < 1) blocks = 1;
  hipStream_t st = (hipStream_t)stream;
  nerf::WgFacts f;
  f.aligned = ldz % 4 == 0 && ldh % 4 == 0 && zc0 % 4 == 0 && hc0 % 4 == 0 && (uintptr_t)dz % 16 == 0 && (uintptr_t)hin % 16 == 0;
  f.hin8 = ldh % 2 == 0 && hc0 % 2 == 0 && (uintptr_t)hin % 8 == 0;
  // the asm-ring form of the small-layer kernels: the point range splits into whole groups of 16 k-steps (32 points) per
  // workgroup (every training shape does: P is a multiple of 64).  List mode needs it (whole 32-point tiles)
  f.ring = n_points % 32 == 0 && ldz < (1ll << 28) && ldh < (1ll << 28);
  f.live = live != nullptr;
  // one 256 x 256 layer on the batched ring launch: whole groups of 8 k-steps and at least one per workgroup of the plain grid
  // (mlp_backward_impl asks for num_cus() / 8 groups instead, whatever the grid: the two tests were written apart and stay apart)
  if (n_out == 256 && n_in == 256 && f.aligned && n_points % 16 == 0 && n_points / 16 >= blocks &&
      ldz * 8 < (1ll << 31) && ldh * 8 < (1ll << 31)) {
    WgradBatch wb;
    wb.job[0] = a; wb.n_jobs = 1;
    return wgrad256_ring(wb, blocks, live, n_live, st);
  }
  const nerf::WgChoice c = nerf::wg_choose(n_out, n_in, f);
  if (c.form == nerf::kWgNoListKernel) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_wgrad: live-tile list on a shape without an asm-ring kernel");
  return wgrad_launch(c, a, dim3((unsigned)blocks), st, std::make_integer_sequence<int, nerf::kWgNumRows>());
}

int32_t nerf_wgrad(const float* dz, int64_t ldz, int32_t zc0, int32_t n_out, const float* hin, int64_t ldh,
                   int32_t hc0, int32_t n_in, float* dw, int64_t ldw, int32_t wc0, float* db, int64_t n_points,
                   void* stream) {
  return wgrad_impl(dz, ldz, zc0, n_out, hin, ldh, hc0, n_in, dw, ldw, wc0, db, n_points, nullptr, nullptr, stream);
}

int32_t nerf_composite_backward(const float* raw, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                                int32_t n_samples, int32_t white_bkgd, const float* g_rgb, const float* g_depth,
                                float* g_raw, float* g_t, void* stream) {
  if (n_rays < 0 || n_samples <= 0 || t_ray_stride < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_backward: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!raw || !tvals || !g_rgb || !g_raw) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_backward: null argument");
  if (n_samples > kCbMaxSamples) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_backward: at most 192 samples per ray");
  return NERF_LAUNCH(nerf_composite_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), (hipStream_t)stream, raw, tvals,
                     (long long)t_ray_stride, (long long)n_rays, n_samples, white_bkgd, g_rgb, g_depth, g_raw, g_t);
}

// the same pair for the backward: nerf_sample_fine_backward and nerf_sample_fine_rays_backward
static int32_t sample_fine_backward(const char* entry, const float* raw_coarse, const float* t_coarse, int64_t t_ray_stride,
                                    const float* u, int64_t u_ray_stride, int64_t n_rays, const float* t_sorted,
                                    const float* g_t_sorted, float* g_raw_coarse, void* stream) {
  if (n_rays == 0) return NERF_OK;
  if (!raw_coarse || !t_coarse || !u || !t_sorted || !g_t_sorted || !g_raw_coarse) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  const dim3 blocks((unsigned)((n_rays + 3) / 4));
  const long long ts = t_ray_stride, us = u_ray_stride, n = n_rays;
  return ts != 0 || us != 0
             ? NERF_LAUNCH(nerf_sample_bwd_kernel<true>, blocks, dim3(256), (hipStream_t)stream, raw_coarse, t_coarse, ts, u, us, n,
                           g_t_sorted, g_raw_coarse)
             : NERF_LAUNCH(nerf_sample_bwd_kernel<false>, blocks, dim3(256), (hipStream_t)stream, raw_coarse, t_coarse, ts, u, us, n,
                           g_t_sorted, g_raw_coarse);
}
int32_t nerf_sample_fine_backward(const float* raw_coarse, const float* t_coarse, const float* u, int64_t n_rays,
                                  const float* t_sorted, const float* g_t_sorted, float* g_raw_coarse, void* stream) {
  if (n_rays < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sample_fine_backward: bad size");
  return sample_fine_backward("nerf_sample_fine_backward", raw_coarse, t_coarse, 0, u, 0, n_rays, t_sorted, g_t_sorted, g_raw_coarse, stream);
}
int32_t nerf_sample_fine_rays_backward(const float* raw_coarse, const float* t_coarse, int64_t t_ray_stride, const float* u,
                                       int64_t u_ray_stride, int64_t n_rays, const float* t_sorted, const float* g_t_sorted,
                                       float* g_raw_coarse, void* stream) {
  if (n_rays < 0 || bad_strides(t_ray_stride, u_ray_stride))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sample_fine_rays_backward: bad size or stride (t: 0 or 64, u: 0 or 128)");
  return sample_fine_backward("nerf_sample_fine_rays_backward", raw_coarse, t_coarse, t_ray_stride, u, u_ray_stride, n_rays, t_sorted,
                              g_t_sorted, g_raw_coarse, stream);
}

int32_t nerf_stratified_samples(const float* t_linear, const float* jitter, int64_t n_rays, float* t_coarse, void* stream) {
  if (n_rays < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_stratified_samples: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!t_linear || !jitter || !t_coarse) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_stratified_samples: null argument");
  const long long ne = (long long)n_rays * NERF_N_SAMPLES;
  return NERF_LAUNCH(nerf_stratified_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), (hipStream_t)stream, t_linear, jitter,
                     (long long)n_rays, t_coarse);
}

int32_t nerf_viewdirs_backward(const float* gsave, int64_t n_rays, int32_t n_samples, const float* w_views,
                               const float* viewdirs, float* g_viewdirs, void* stream) {
  if (n_rays < 0 || n_samples <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_viewdirs_backward: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!gsave || !w_views || !viewdirs || !g_viewdirs) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_viewdirs_backward: null argument");
  if (n_rays > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_viewdirs_backward: too many rays for one launch");
  return NERF_LAUNCH(nerf_viewdirs_bwd_kernel, dim3((unsigned)n_rays), dim3(128), (hipStream_t)stream,
                     gsave + TrainGrad::off_gzv(n_rays * n_samples), (long long)n_rays, n_samples, w_views, viewdirs, g_viewdirs);
}

int32_t nerf_rays_viewdirs_backward(const float* rays_d, int64_t n_rays, int32_t n_samples, const float* gsave,
                                    const float* w_views, float* g_rays_d_view, void* stream) {
  if (n_rays < 0 || n_samples <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_rays_viewdirs_backward: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!rays_d || !gsave || !w_views || !g_rays_d_view) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_rays_viewdirs_backward: null argument");
  if (n_rays > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_rays_viewdirs_backward: too many rays for one launch");
  const long long P = n_rays * n_samples;
  return NERF_LAUNCH(nerf_rays_viewdirs_bwd_kernel, dim3((unsigned)n_rays), dim3(128), (hipStream_t)stream,
                     gsave + TrainGrad::off_gzv(P), reinterpret_cast<const int*>(gsave + TrainGrad::off_flags(P)),
                     reinterpret_cast<const int*>(gsave + TrainGrad::off_count(P)), n_samples, w_views, rays_d, g_rays_d_view);
}

int32_t nerf_rays_backward(int64_t n_rays, const float* t_coarse, int64_t t_ray_stride, const float* g_x_coarse,
                           const float* t_sorted, const float* g_x_fine, const float* g_rays_d_view, float* g_rays_o,
                           float* g_rays_d, void* stream) {
  if (n_rays < 0 || (t_ray_stride != 0 && t_ray_stride != NERF_N_SAMPLES))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_rays_backward: bad size or stride (t: 0 or 64)");
  if (n_rays == 0) return NERF_OK;
  if (!g_rays_o || !g_rays_d || (g_x_coarse && !t_coarse) || (g_x_fine && !t_sorted))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_rays_backward: null argument");
  const long long blocks = (n_rays + 3) / 4;
  if (blocks > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_rays_backward: too many rays for one launch");
  return NERF_LAUNCH(nerf_rays_bwd_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, (long long)n_rays, t_coarse,
                     (long long)t_ray_stride, g_x_coarse, t_sorted, g_x_fine, g_rays_d_view, g_rays_o, g_rays_d);
}

int32_t nerf_adam_step(int32_t n_tensors, float* const params[], const float* const grads[], float* const exp_avg[],
                       float* const exp_avg_sq[], const int64_t numel[], float lr, float beta1, float beta2, float eps,
                       float weight_decay, float clip_value, int64_t step, void* stream) {
  if (n_tensors <= 0 || n_tensors > kAdamMaxTensors || step <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: bad size");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: null argument");
  AdamArgs a;
  long long run = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || numel[i] < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: null tensor");
    a.p[i] = params[i]; a.g[i] = grads[i]; a.m[i] = exp_avg[i]; a.v[i] = exp_avg_sq[i];
    run += numel[i]; a.end[i] = run;
  }
  if (run == 0) return NERF_OK;
  a.n_tensors = n_tensors; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.clip = clip_value;
  a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  long long blocks = (run + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  return NERF_LAUNCH(nerf_adam_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, a);
}

int64_t nerf_train_grad_floats(int64_t n_points) { return n_points < 0 ? -1 : TrainGrad::floats(n_points); }
int64_t nerf_train_live_count_offset(int64_t n_points) { return n_points < 0 ? -1 : TrainGrad::off_count(n_points); }
int64_t nerf_packed_bwd_bytes(int32_t precision) {
  if (precision == NERF_PREC_F32) return nerf::kBwdPackedFloats * (int64_t)sizeof(float);
  if (precision == NERF_PREC_F32X) return nerf::kXbPackedBytes;
  return -1;
}

int32_t nerf_pack_model_bwd(const float* const params[24], void* packed_bwd_v, int32_t precision, void* stream) {
  PackArgs a;
  if (const int rc = fill_pack_args("nerf_pack_model_bwd", params, packed_bwd_v, a)) return rc;
  if (precision == NERF_PREC_F32X) {
    const long long n = nerf::kF16ConstBytes / 4 + (long long)nerf::kXbSteps * 512;
    return NERF_LAUNCH(nerf_pack_bwd_f32x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), (hipStream_t)stream, a);
  }
  if (precision != NERF_PREC_F32) return fail(NERF_ERR_UNSUPPORTED, "%s", "nerf_pack_model_bwd: f32 or f32x only");
  return NERF_LAUNCH(nerf_pack_bwd_kernel, dim3((unsigned)((nerf::kBwdPackedFloats + 255) / 256)), dim3(256), (hipStream_t)stream, a);
}

// grads[24]: device pointers in state_dict order (nn.Linear layouts), accumulated into (caller zeroes them); nullptr: the
// data-gradient chain alone (a frozen network: no weight-gradient launch, nothing to poison)
// shared by the ray-mode and the point-mode entry: data-gradient chain, then the weight / bias gradients
// occupied (masked backward, point mode on compact rows): device count M of the rows the forward filled.  Tiles behind row
// M - 1 hold nothing, so a live-tile list is built even with NERF_DEAD_TILE_SKIP=0 -- then of every occupied tile.
static int32_t mlp_backward_impl(const BwdArgs& a_in, bool pts_mode, float* const grads[24], int32_t precision, void* stream,
                                 const int* occupied = nullptr) {
  // density only: both chains skip the colour branch in the kernel (ray mode), and its three weight-gradient jobs are skipped
  // here: their result is exactly zero
  BwdArgs a = a_in;
  // ray mode with g_x: the chain writes g_x through its one output pointer (BwdArgs::g_t, bit 0 set), g_t follows from it
  float* const g_t_out = a.g_t;
  float* const g_x_out = a.g_x;
  const bool ray_x = !pts_mode && g_x_out != nullptr;
  if (ray_x) {
    a.g_t = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(g_x_out) | 1);
    a.g_x = nullptr;
  }
  const bool dens = a.density_only != 0;
  const long long P = a.n_points;
  const float* draw = a.draw; const float* save = a.save; float* gsave = a.gsave;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  // live tiles: tiles whose incoming gradient is zero throughout are dropped from the chain launch and from every
  // weight-gradient launch -- see nerf_tile_flags_kernel.  Needs the asm-ring weight-gradient kernels (whole 32-point tiles).
  // NERF_DEAD_TILE_SKIP=0 in the environment turns it off (tests compare the two).
  const int* live = nullptr; const int* n_live = nullptr;
  {
    const bool by_gradient = dead_tile_list_available(P, precision);
    if (by_gradient || occupied) {
      int* flags = reinterpret_cast<int*>(gsave + TrainGrad::off_flags(P));
      int* lv = reinterpret_cast<int*>(gsave + TrainGrad::off_live(P));
      int* cnt = reinterpret_cast<int*>(gsave + TrainGrad::off_count(P));
      rc = by_gradient ? NERF_LAUNCH(nerf_tile_flags_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), st,
                                     reinterpret_cast<const f32x4*>(draw), P, a.density_only, flags)
                       : NERF_LAUNCH(nerf_tile_occupied_kernel, dim3((unsigned)((P / 32 + 255) / 256)), dim3(256), st, occupied, P / 32,
                                     flags);
      if (rc) return rc;
      if ((rc = NERF_LAUNCH(nerf_tile_scan_kernel, dim3(1), dim3(kScanThreads), st, flags, (int)(P / 32), lv, cnt))) return rc;
      // dead tiles have no workgroup: their g_t / g_x is the zero written here
      if (!pts_mode && !ray_x && g_t_out && hipMemsetAsync(g_t_out, 0, (size_t)P * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return fail(NERF_ERR_HIP, "%s", "nerf_mlp_backward: memset failed");
      if (g_x_out && hipMemsetAsync(g_x_out, 0, (size_t)P * 3 * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return fail(NERF_ERR_HIP, "%s", "nerf_mlp_backward: memset failed");
      // point mode has one more consumer of gsave: nerf_viewdirs_backward sums the g_zv rows of ALL samples of a ray, dead
      // tiles included -- their rows are the zeros written here (ray mode: nerf_rays_viewdirs_backward skips dead tiles by their flag)
      // (masked backward: its g_zv rows are read by the weight-gradient kernels alone, live tiles only)
      if (pts_mode && !occupied && hipMemsetAsync(gsave + TrainGrad::off_gzv(P), 0, (size_t)TrainSave::pad32(P) * 128 * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return fail(NERF_ERR_HIP, "%s", "nerf_mlp_backward: memset failed");
      live = lv; n_live = cnt;
      a.live_tiles = lv; a.n_live = cnt;
    } else {
      if (hipMemsetAsync(gsave + TrainGrad::off_count(P), 0xFF, sizeof(int), (hipStream_t)stream) != hipSuccess)   // count = -1: no list
        return fail(NERF_ERR_HIP, "%s", "nerf_mlp_backward: memset failed");
      // a dense backward needs every row of `save`: refuse (NaN in the alpha-bias gradient) a buffer whose forward skipped rows
      // (chain only: the skipped tiles' incoming gradient is zero by the forward's contract, so is all the chain makes of them)
      if (grads && (rc = NERF_LAUNCH(nerf_check_stamp_kernel, dim3(1), dim3(64), st, save + TrainSave::off_stamp(P),
                                     grads[nerf::P_BA]))) return rc;
    }
  }
  if (precision == NERF_PREC_F32X) {
    const dim3 blocks(persistent_blocks(P, kXTilePts)), threads(kXThreads);
    rc = pts_mode ? NERF_LAUNCH(nerf_mlp_bwd_f32x_kernel<true>, blocks, threads, st, a)
         : dens   ? NERF_LAUNCH((nerf_mlp_bwd_f32x_kernel<false, true>), blocks, threads, st, a)
                  : NERF_LAUNCH(nerf_mlp_bwd_f32x_kernel<false>, blocks, threads, st, a);
  } else if (precision == NERF_PREC_F32) {
    const long long tiles = (P + nerf::kTilePts - 1) / nerf::kTilePts;
    if (tiles > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward: too many points for one launch");
    // barrier-free: one-wave workgroups (with a live list: one slot per tile, slots >= *n_live exit at once)
    rc = pts_mode ? NERF_LAUNCH(nerf_mlp_bwd_f32_kernel<true>, dim3((unsigned)tiles), dim3(64), st, a)
                  : NERF_LAUNCH(nerf_mlp_bwd_f32_kernel<false>, dim3((unsigned)tiles), dim3(64), st, a);
  } else return fail(NERF_ERR_UNSUPPORTED, "%s", "nerf_mlp_backward: f32 or f32x only");
  if (rc) return rc;
  if (ray_x && g_t_out &&
      (rc = NERF_LAUNCH(nerf_gt_of_gx_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), st, g_x_out, a.rays_d, a.n_samples, P,
                        g_t_out)))
    return rc;
  if (!grads) return NERF_OK;                       // chain only
  // weight / bias gradients: grad_W = g_z^T @ input, grad_b = sum g_z   (network.py:22-47 layers)
  const float* pe = save + TrainSave::off_pe(P);
  const float* dpe = save + TrainSave::off_dpe(P);
  auto H = [&](int l) { return save + TrainSave::off_h(P, l); };
  auto GZ = [&](int l) { return gsave + TrainGrad::off_gz(P, l); };
  const float* f = save + TrainSave::off_f(P);
  const float* hv = save + TrainSave::off_hv(P);
  const float* gzv = gsave + TrainGrad::off_gzv(P);
  const float* gf = gsave + TrainGrad::off_gf(P);
  using namespace nerf;
#define WG(...) do { rc = wgrad_impl(__VA_ARGS__, P, live, n_live, stream); if (rc) return rc; } while (0)
  // density only: the gradients of rgb_linear, views_linears.0 and feature_linear are identically zero (left as zeroed by the caller)
  if (!dens) WG(draw, 4, 0, 3, hv, 128, 0, 128, grads[P_WR], 128, 0, grads[P_BR]);      // rgb_linear
  WG(draw, 4, 3, 1, H(7), 256, 0, 256, grads[P_WA], 256, 0, grads[P_BA]);               // alpha_linear
  if (!dens) {
    WG(gzv, 128, 0, 128, f, 256, 0, 256, grads[P_WV], 283, 0, grads[P_BV]);             // views_linears.0 [feature | dirs]
    WG(gzv, 128, 0, 128, dpe, 32, 0, 27, grads[P_WV], 283, 256, nullptr);
  }
  WG(GZ(5), 256, 0, 256, pe, 64, 0, 63, grads[10], 319, 0, grads[11]);                  // skip layer, PE part (+ bias)
  WG(GZ(0), 256, 0, 256, pe, 64, 0, 63, grads[P_W0], 63, 0, grads[P_B0]);
  // the eight 256 x 256 blocks: feature_linear (unless density only), then layers 7..1 with the skip layer's hidden part
  struct { const float* dz; const float* hin; float* dw; int ldw, wc0; float* db; } job[8];
  int n_jobs = 0;
  if (!dens) job[n_jobs++] = {gf, H(7), grads[P_WF], 256, 0, grads[P_BF]};
  for (int l = 7; l >= 1; --l) {
    if (l == 5) job[n_jobs++] = {GZ(5), H(4), grads[10], 319, 63, nullptr};
    else job[n_jobs++] = {GZ(l), H(l - 1), grads[2 * l], 256, 0, grads[2 * l + 1]};
  }
  if (precision == NERF_PREC_F32X) {
    // in one launch on the bf16x3 path (nerf_wgrad_bf16x3.hip.inc)
    WgradXArgs w;
    w.n_points = P; w.n_jobs = n_jobs; w.live_tiles = live; w.n_live = n_live;
    for (int i = 0; i < n_jobs; ++i) {
      WgradXJob& j = w.job[i];
      j.dz = job[i].dz; j.hin = job[i].hin; j.dw = job[i].dw; j.db = job[i].db; j.ldw = job[i].ldw; j.wc0 = job[i].wc0;
      j.ldz = 256; j.zc0 = 0; j.ldh = 256; j.hc0 = 0;                                  // ld 256: the kernel assumes 1-KiB rows
    }
    const long long steps = (P + 15) / 16;
    long long slices = num_cus() / n_jobs;
    if (slices > steps) slices = steps;
    if (slices < 1) slices = 1;
    return NERF_LAUNCH(nerf_wgrad256_bf16x3_kernel, dim3((unsigned)(slices * n_jobs)), dim3(256), st, w);
  } else if (P % 16 == 0 && P / 16 >= num_cus() / 8) {
    // fp32 MFMA, in one launch of the ring kernel (a test on the point count alone, where wgrad_impl's is on its own grid: the
    // two were written apart and stay apart; below it the layers go one by one, through wgrad_impl's test)
    WgradBatch wb;
    wb.n_jobs = n_jobs;
    for (int i = 0; i < n_jobs; ++i) {
      WgradArgs& j = wb.job[i];
      j.dz = job[i].dz; j.ldz = 256; j.zc0 = 0; j.hin = job[i].hin; j.ldh = 256; j.hc0 = 0;
      j.dw = job[i].dw; j.ldw = job[i].ldw; j.wc0 = job[i].wc0; j.db = job[i].db; j.n_points = P;
    }
    long long slices = num_cus() / n_jobs;
    if (slices < 1) slices = 1;                       // a device with fewer CUs than jobs still gets a non-empty grid
    return wgrad256_ring(wb, slices, live, n_live, st);
  } else {
    for (int i = 0; i < n_jobs; ++i) WG(job[i].dz, 256, 0, 256, job[i].hin, 256, 0, 256, job[i].dw, job[i].ldw, job[i].wc0, job[i].db);
  }
#undef WG
  return NERF_OK;
}

// the ray-mode backward entries (grads == nullptr where `grads_optional`: the chain alone)
static int32_t backward_rays(const char* entry, const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                             int64_t n_rays, int32_t n_samples, const void* packed_bwd_v, const float* draw, const float* save,
                             float* gsave, float* g_t, float* g_x, float* const grads[24], bool grads_optional, bool density_only,
                             int32_t precision, void* stream) {
  if (n_rays < 0 || n_samples <= 0 || t_ray_stride < 0) return fail(NERF_ERR_INVALID_ARG, "%s: bad size", entry);
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !tvals || !packed_bwd_v || !draw || !save || !gsave || (!grads && !grads_optional))
    return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (grads)
    for (int i = 0; i < 24; ++i) if (!grads[i]) return fail(NERF_ERR_INVALID_ARG, "%s: null gradient pointer", entry);
  BwdArgs a{};
  a.rays_o = rays_o; a.rays_d = rays_d; a.tvals = tvals; a.t_ray_stride = t_ray_stride; a.n_points = n_rays * n_samples;
  a.n_samples = n_samples; a.packed_bwd = (const float*)packed_bwd_v; a.draw = draw; a.save = save; a.gsave = gsave; a.g_t = g_t;
  a.g_x = g_x; a.density_only = density_only;
  return mlp_backward_impl(a, false, grads, precision, stream);
}

int32_t nerf_mlp_backward(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                          int64_t n_rays, int32_t n_samples, const void* packed_bwd_v, const float* draw,
                          const float* save, float* gsave, float* g_t, float* const grads[24], int32_t precision,
                          void* stream) {
  return backward_rays("nerf_mlp_backward", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed_bwd_v, draw, save, gsave,
                       g_t, nullptr, grads, false, false, precision, stream);
}

int32_t nerf_mlp_backward_density(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                  int64_t n_rays, int32_t n_samples, const void* packed_bwd_v, const float* draw,
                                  const float* save, float* gsave, float* g_t, float* const grads[24], int32_t precision,
                                  void* stream) {
  return backward_rays("nerf_mlp_backward_density", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed_bwd_v, draw, save,
                       gsave, g_t, nullptr, grads, false, true, precision, stream);
}

int32_t nerf_mlp_backward_rays_x(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                 int64_t n_rays, int32_t n_samples, const void* packed_bwd_v, const float* draw,
                                 const float* save, float* gsave, float* g_t, float* g_x, float* const grads[24],
                                 int32_t density_only, int32_t precision, void* stream) {
  return backward_rays("nerf_mlp_backward_rays_x", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed_bwd_v, draw, save,
                       gsave, g_t, g_x, grads, true, density_only != 0, precision, stream);
}

int32_t nerf_mlp_backward_points(const float* pts, int64_t n_rays, int32_t n_samples, const void* packed_bwd_v,
                                 const float* draw, const float* save, float* gsave, float* g_pts,
                                 float* const grads[24], int32_t precision, void* stream) {
  if (n_rays < 0 || n_samples <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward_points: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!pts || !packed_bwd_v || !draw || !save || !gsave || !grads)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward_points: null argument");
  for (int i = 0; i < 24; ++i) if (!grads[i]) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward_points: null gradient pointer");
  BwdArgs a{};
  a.pts = pts; a.g_x = g_pts; a.n_points = n_rays * n_samples; a.n_samples = n_samples;
  a.packed_bwd = (const float*)packed_bwd_v; a.draw = draw; a.save = save; a.gsave = gsave;
  return mlp_backward_impl(a, true, grads, precision, stream);
}

int64_t nerf_train_save_floats(int64_t n_points) { return n_points < 0 ? -1 : TrainSave::floats(n_points); }

int32_t nerf_mlp_forward_rays_save(const float* rays_o, const float* rays_d, const float* tvals,
                                   int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                   const void* packed, float* raw, float* save, int32_t precision, void* stream) {
  return forward_rays("nerf_mlp_forward_rays_save", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed, raw, true, save,
                      false, false, precision, stream);
}
int32_t nerf_mlp_forward_rays_save_for_compositing(const float* rays_o, const float* rays_d, const float* tvals,
                                                   int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                                   const void* packed, float* raw, float* save, int32_t precision, void* stream) {
  return forward_rays("nerf_mlp_forward_rays_save_for_compositing", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed,
                      raw, true, save, false, true, precision, stream);
}
int32_t nerf_mlp_forward_rays_save_density(const float* rays_o, const float* rays_d, const float* tvals,
                                           int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                           const void* packed, float* raw, float* save, int32_t precision, void* stream) {
  return forward_rays("nerf_mlp_forward_rays_save_density", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed, raw, true,
                      save, true, false, precision, stream);
}

// ---- masked (fast_sampling) fine pass of a training step
static bool masked_sizes_ok(int64_t n_rays, int32_t n_samples, int64_t t_ray_stride) {
  return n_rays >= 0 && n_samples > 0 && t_ray_stride >= 0 && n_rays <= (int64_t)0x7fffffff / n_samples;     // point ids are int32
}
int64_t nerf_compact_valid_workspace_bytes(int64_t n_points) {
  if (n_points < 0 || n_points > 0x7fffffffLL) return -1;
  return align256(((n_points + kCompactBlock - 1) / kCompactBlock) * (int64_t)sizeof(int));
}
int32_t nerf_compact_valid(const uint8_t* valid, int64_t n_points, int32_t* index, int32_t* count, void* workspace, void* stream) {
  if (n_points < 0 || n_points > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_compact_valid: point ids are int32");
  if (!count) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_compact_valid: null argument");
  hipStream_t st = (hipStream_t)stream;
  if (n_points == 0) {
    if (hipMemsetAsync(count, 0, sizeof(int), st) != hipSuccess) return fail(NERF_ERR_HIP, "%s", "nerf_compact_valid: memset failed");
    return NERF_OK;
  }
  if (!valid || !index || !workspace) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_compact_valid: null argument");
  const long long n_blocks = (n_points + kCompactBlock - 1) / kCompactBlock;
  int* block = (int*)workspace;
  int rc = NERF_LAUNCH(nerf_compact_count_kernel, dim3((unsigned)n_blocks), dim3(kCompactBlock), st, valid, (long long)n_points, block);
  if (rc) return rc;
  if ((rc = NERF_LAUNCH(nerf_compact_scan_kernel, dim3(1), dim3(kScanThreads), st, block, n_blocks, count))) return rc;
  return NERF_LAUNCH(nerf_compact_scatter_kernel, dim3((unsigned)n_blocks), dim3(kCompactBlock), st, valid, (long long)n_points, block,
                     index);
}

int32_t nerf_mlp_forward_rays_save_masked(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                          int64_t n_rays, int32_t n_samples, const int32_t* index, const int32_t* count,
                                          const void* packed, float* raw, float* save, int32_t precision, void* stream) {
  if (!masked_sizes_ok(n_rays, n_samples, t_ray_stride)) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_forward_rays_save_masked: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!index || !count) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_forward_rays_save_masked: null argument");
  // the fine pass of a step: `raw` goes to compositing, so the rule of nerf_mlp_forward_rays_save_for_compositing holds per
  // compact tile
  return forward_rays("nerf_mlp_forward_rays_save_masked", rays_o, rays_d, tvals, t_ray_stride, n_rays, n_samples, packed, raw, true,
                      save, false, true, precision, stream, index, count);
}

// The workspace of nerf_mlp_backward_masked: the compact rows the chain works on (incoming gradient, points) and its g_x rows
struct MaskedBackwardWorkspace {
  float* draw_c; float* pts_c; float* gx_c;
  int64_t bytes;
  MaskedBackwardWorkspace(const void* base, int64_t P) {
    Carver c(base);
    draw_c = c.take<float>(P * 4);
    pts_c = c.take<float>(P * 3);
    gx_c = c.take<float>(P * 3);
    bytes = c.bytes();
  }
};
int64_t nerf_mlp_backward_masked_workspace_bytes(int64_t n_points) {
  if (n_points < 0 || n_points > 0x7fffffffLL) return -1;
  return MaskedBackwardWorkspace(nullptr, n_points).bytes;
}
int32_t nerf_mlp_backward_masked(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                 int64_t n_rays, int32_t n_samples, const int32_t* index, const int32_t* count,
                                 const void* packed_bwd_v, const float* draw, const float* save, float* gsave, float* g_t,
                                 float* const grads[24], int32_t precision, void* workspace, void* stream) {
  if (!masked_sizes_ok(n_rays, n_samples, t_ray_stride)) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward_masked: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !tvals || !index || !count || !packed_bwd_v || !draw || !save || !gsave || !grads || !workspace)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward_masked: null argument");
  for (int i = 0; i < 24; ++i) if (!grads[i]) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_backward_masked: null gradient pointer");
  if (precision != NERF_PREC_F32 && precision != NERF_PREC_F32X) return fail(NERF_ERR_UNSUPPORTED, "%s", "nerf_mlp_backward_masked: f32 or f32x only");
  const long long P = n_rays * (int64_t)n_samples;
  // compact rows past the count are kept out by the live-tile list alone: the list-mode kernels must exist (whole 32-point tiles)
  if (P % 32 != 0)
    return fail(NERF_ERR_UNSUPPORTED, "%s", "nerf_mlp_backward_masked: needs the live-tile kernels and a point count that is a multiple of 32");
  hipStream_t st = (hipStream_t)stream;
  const MaskedBackwardWorkspace w(workspace, P);
  const unsigned blocks = (unsigned)((P + 255) / 256);
  int rc = NERF_LAUNCH(nerf_masked_gather_kernel, dim3(blocks), dim3(256), st, index, count, P, reinterpret_cast<const f32x4*>(draw),
                       rays_o, rays_d, tvals, (long long)t_ray_stride, n_samples, reinterpret_cast<f32x4*>(w.draw_c), w.pts_c);
  if (rc) return rc;
  // the chain and the weight-gradient kernels in point mode over the compact rows (live tiles only)
  BwdArgs a{};
  a.pts = w.pts_c; a.g_x = g_t ? w.gx_c : nullptr; a.n_points = P; a.n_samples = n_samples;
  a.packed_bwd = (const float*)packed_bwd_v; a.draw = w.draw_c; a.save = save; a.gsave = gsave;
  rc = mlp_backward_impl(a, true, grads, precision, stream, count);
  if (rc || !g_t) return rc;
  if (hipMemsetAsync(g_t, 0, (size_t)P * sizeof(float), st) != hipSuccess) return fail(NERF_ERR_HIP, "%s", "nerf_mlp_backward_masked: memset failed");
  return NERF_LAUNCH(nerf_masked_gt_scatter_kernel, dim3(blocks), dim3(256), st, index, count, P, w.gx_c, rays_d, n_samples, g_t);
}

int32_t nerf_mlp_forward_points_save(const float* pts, const float* viewdirs, int64_t n_rays, int32_t n_samples,
                                     const void* packed, float* raw, float* save, int32_t precision, void* stream) {
  if (n_rays < 0 || n_samples <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_forward_points_save: bad size");
  if (n_rays == 0) return NERF_OK;
  if (!pts || !viewdirs || !packed || !raw || !save) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mlp_forward_points_save: null argument");
  MlpArgs a{};
  a.pts = pts; a.viewdirs = viewdirs; a.n_points = n_rays * n_samples; a.n_samples = n_samples;
  a.packed = (const float*)packed; a.raw = raw; a.save = save;
  if (hipMemsetAsync(save + TrainSave::off_stamp(a.n_points), 0, 4 * sizeof(float), (hipStream_t)stream) != hipSuccess)      // every row stored
    return fail(NERF_ERR_HIP, "%s", "nerf_mlp_forward_points_save: memset failed");
  return launch_mlp(a, false, true, precision, (hipStream_t)stream, "nerf_mlp_forward_points_save");
}

int32_t nerf_image_ssim(const float* pred, const float* gt, int32_t H, int32_t W, double* sum1, void* stream) {
  if (H < 7 || W < 7) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_image_ssim: image smaller than the 7x7 window");
  if (!pred || !gt || !sum1) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_image_ssim: null argument");
  if (hipMemsetAsync(sum1, 0, sizeof(double), (hipStream_t)stream) != hipSuccess)
    return fail(NERF_ERR_HIP, "%s", "nerf_image_ssim: memset failed");
  long long blocks = ((long long)(H - 6) * (W - 6) * 3 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  return NERF_LAUNCH(nerf_ssim_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, pred, gt, H, W, sum1);
}

// Ray blocks.  nerf_render_forward walks a frame in blocks of kRenderBlockRays rays (the four stages per block, same stream): the
// intermediates -- raw_coarse, t_sorted, raw_fine: 4864 B per ray -- belong to ONE block, so the workspace is bounded (5.1 GB) whatever
// the frame (round 2: 12.5 GB at 1600x1600, growing with the frame).  Rays are independent: the image is bit-identical to the one-block
// render (tests).  The block is LARGE on purpose: with 65 536-ray blocks (320 MB, Infinity-Cache-resident intermediates) the fp32
// frame lost 0.2 % and the fp16 frame 5 % (134.7 -> 141.4 ms at 800x800) -- every block pays the persistent kernels' pipeline fill and
// tail, and the far-plane guard's launch (one point per ray) fills 2 tiles per CU -- while nothing is gained from the cache
// residency: the MLP launches are matrix-bound and HBM sits at < 1 % of its bandwidth either way.  NERF_RENDER_BLOCK_RAYS in the
// environment overrides the block size (A/B, tests).
static constexpr int64_t kRenderBlockRays = 1 << 20;
static int64_t render_block_rays() {
  const char* env = getenv("NERF_RENDER_BLOCK_RAYS");
  // capped at the rays whose 192 point ids fit in int32: a larger block would switch the fp16 far-plane guard off (render_frame)
  constexpr long long kMax = 0x7fffffff / (NERF_N_SAMPLES + NERF_N_IMPORTANCE);
  if (env) { const long long v = atoll(env); if (v >= 64) return (int64_t)(v < kMax ? v : kMax); }
  return kRenderBlockRays;
}

// The workspace of one block of `n_rays` rays, carved in this order, every piece 256-byte aligned.  index / count: with fast_sampling
// the compacted ids of the valid merged samples and their number (and, once that list is consumed, the guard's), otherwise the
// last-sample ids of the fp16 far-plane guard and their number.  t_jit: the jittered coarse depths [n,64] of a stochastic render.  occupancy (nerf_render_forward_occupancy): the
// fine pass may be listed without fast_sampling too, and the coarse pass gets a mask [n,64] and an id list of its own behind.
struct RenderWorkspace {
  float* raw_c; float* t_sorted = nullptr; float* raw_f = nullptr; uint8_t* valid = nullptr; int* index; int* count; float* t_jit = nullptr;
  uint8_t* valid_c = nullptr; int* index_c = nullptr;
  int64_t bytes;
  RenderWorkspace(void* base, int64_t n_rays, int32_t n_importance, int32_t fast_sampling, bool stochastic, bool occupancy = false) {
    Carver c(base);
    const int64_t S = NERF_N_SAMPLES + NERF_N_IMPORTANCE;
    raw_c = c.take<float>(n_rays * NERF_N_SAMPLES * 4);
    if (n_importance) {
      t_sorted = c.take<float>(n_rays * S);
      raw_f = c.take<float>(n_rays * S * 4);
    }
    if (n_importance && (fast_sampling || occupancy)) {
      valid = c.take<uint8_t>(n_rays * S);
      index = c.take<int>(n_rays * S);
    } else {
      index = c.take<int>(n_rays);
    }
    count = c.take<int>(1);
    if (stochastic) t_jit = c.take<float>(n_rays * NERF_N_SAMPLES);
    if (occupancy) {
      valid_c = c.take<uint8_t>(n_rays * NERF_N_SAMPLES);
      index_c = c.take<int>(n_rays * NERF_N_SAMPLES);
    }
    bytes = c.bytes();
  }
};
static int64_t render_workspace_bytes(int64_t n_rays_frame, int32_t n_importance, int32_t fast_sampling, bool stochastic,
                                      bool occupancy = false) {
  if (n_rays_frame < 0) return -1;
  const int64_t n_rays = n_rays_frame < render_block_rays() ? n_rays_frame : render_block_rays();
  return RenderWorkspace(nullptr, n_rays, n_importance, fast_sampling, stochastic, occupancy).bytes;
}

// Occupancy culling of a frame (nerf_render_forward_occupancy, csrc/nerf_occupancy.hip.inc): the bitfields of the coarse and the fine
// pass (each nullable: that pass runs on every sample), the lookup frame, and the DEVICE int64[2] that takes the numbers of coarse /
// fine points evaluated (nullable).
struct RenderOccupancy {
  const uint32_t* coarse; const uint32_t* fine;
  int32_t dims[3]; float box_min[3], inv_step[3];
  long long* evaluated;
};
static int occupancy_tally(const int* count, long long all, long long* evaluated, hipStream_t st);
int64_t nerf_render_workspace_bytes(int64_t n_rays_frame, int32_t n_importance, int32_t fast_sampling) {
  return render_workspace_bytes(n_rays_frame, n_importance, fast_sampling, false);
}
int64_t nerf_render_stochastic_workspace_bytes(int64_t n_rays_frame, int32_t n_importance) {
  return render_workspace_bytes(n_rays_frame, n_importance, 0, true);
}

// One frame, block by block through the four stages.  jitter / u_rays (stochastic render: task == "train", no grad) give every ray
// its own coarse depths (nerf_stratified_samples of the block, stride 64) and its own u (stride 128); without them the shared
// tables go through with stride 0, and nerf_sample_fine_rays then launches nerf_sample_fine_kernel.
static int32_t render_frame(const char* entry, const float* rays_o, const float* rays_d, int64_t n_rays, const void* packed_coarse,
                            const void* packed_fine, const float* t_coarse, const float* u, const float* jitter, const float* u_rays,
                            bool stochastic, int32_t n_importance, int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                            float weights_threshold, void* workspace, int64_t workspace_bytes, float* rgb, float* depth, void* stream,
                            const RenderOccupancy* occ = nullptr) {
  if (n_rays < 0) return fail(NERF_ERR_INVALID_ARG, "%s: bad size", entry);
  if (n_importance != 0 && n_importance != NERF_N_IMPORTANCE)
    return fail(NERF_ERR_INVALID_ARG, "%s: n_importance must be 0 or 128", entry);
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !packed_coarse || !t_coarse || !rgb || !depth || !workspace ||
      (n_importance && (!packed_fine || !u)))
    return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (workspace_bytes < render_workspace_bytes(n_rays, n_importance, fast_sampling, stochastic, occ != nullptr))
    return fail(NERF_ERR_WORKSPACE, "%s: workspace too small", entry);
  // the masked fine pass addresses (ray, sample) pairs by 32-bit ids (nerf_compact_kernel, MlpArgs::index)
  const int64_t S = NERF_N_SAMPLES + NERF_N_IMPORTANCE;
  if (fast_sampling && n_importance && n_rays > (int64_t)0x7fffffff / S)
    return fail(NERF_ERR_INVALID_ARG, "%s: fast_sampling handles at most 11 184 810 rays per call "
                                      "(n_rays * 192 point ids must fit in int32): split the frame", entry);
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = render_block_rays();
  for (int64_t r0 = 0; r0 < n_rays; r0 += B) {
    const int64_t nb = n_rays - r0 < B ? n_rays - r0 : B;
    const float* o = rays_o + 3 * r0;
    const float* d = rays_d + 3 * r0;
    float* rgb_b = rgb + 3 * r0;
    float* depth_b = depth + r0;
    const RenderWorkspace w(workspace, nb, n_importance, fast_sampling, stochastic, occ != nullptr);
    // A pass on a list: the ids with valid != 0 compacted (unordered: `raw` is written by id), `raw` zero-filled -- an unlisted
    // sample keeps raw = 0, and compositing and the sampler both apply relu(sigma), so that is exact wherever its true sigma <= 0
    auto list_pass = [&](const uint8_t* valid, long long np, int* index, float* raw) -> int {
      if (hipMemsetAsync(w.count, 0, sizeof(int), st) != hipSuccess ||
          hipMemsetAsync(raw, 0, (size_t)(np * 4 * (int64_t)sizeof(float)), st) != hipSuccess)
        return fail(NERF_ERR_HIP, "%s: memset failed", entry);
      return NERF_LAUNCH(nerf_compact_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), st, valid, np, index, w.count);
    };
    // (occupancy) the points a pass evaluated: the length of its list, or all of them
    auto tally = [&](int pass, bool listed, long long all) -> int {
      return occ && occ->evaluated ? occupancy_tally(listed ? w.count : nullptr, all, occ->evaluated + pass, st) : NERF_OK;
    };
    const float* tc = t_coarse;
    int64_t tcs = 0;
    int rc;
    if (jitter) {
      rc = nerf_stratified_samples(t_coarse, jitter + NERF_N_SAMPLES * r0, nb, w.t_jit, stream);
      if (rc) return rc;
      tc = w.t_jit; tcs = NERF_N_SAMPLES;
    }
    // hierarchical render: the coarse network only places the fine samples -- nothing but its sigma is read
    // (volume_renderer.py:335; the returned rgb/depth come from the fine outputs, :414-437), so the coarse pass stops after
    // the sigma head.  With n_importance == 0 the coarse outputs ARE the frame and the full network runs.
    const bool cull_c = occ && occ->coarse;
    if (cull_c) {
      rc = nerf_occupancy_mark(o, d, tc, tcs, nb, NERF_N_SAMPLES, occ->coarse, occ->dims, occ->box_min, occ->inv_step, 0, w.valid_c, stream);
      if (rc) return rc;
      rc = list_pass(w.valid_c, nb * NERF_N_SAMPLES, w.index_c, w.raw_c);
      if (rc) return rc;
    }
    // fp16 with fast_sampling: the coarse sigma also DECIDES -- the ESS / ERT mask compares the coarse weights with thresholds, and a
    // weight that crosses one keeps or drops all the fine samples in front of a surface.  With the fp16 coarse sigma the masked render
    // stood at 41-47 dB against the masked f32 render where the plain one stands at 54-58, single rays 1.1 off in depth; so the
    // density pass of that combination runs on the split-fp16 stream behind the packed model (fp32-accurate, as the guard below):
    // 54-88 dB, no ray above 0.27.  It costs the masked fp16 frame 91.5 -> 151.6 ms at 800x800 (LAB_NOTEBOOK).
    const bool fp16 = precision == NERF_PREC_F16 || precision == NERF_PREC_F16S;
    const bool exact_coarse = fp16 && fast_sampling && n_importance;
    rc = forward_rays(entry, o, d, tc, tcs, nb, NERF_N_SAMPLES, exact_coarse ? (const char*)packed_coarse + nerf::kF16PackedBytes : packed_coarse,
                      w.raw_c, false, nullptr, n_importance != 0, false, exact_coarse ? NERF_PREC_F32X : precision, stream,
                      cull_c ? w.index_c : nullptr, cull_c ? w.count : nullptr);
    if (rc) return rc;
    rc = tally(0, cull_c, nb * NERF_N_SAMPLES);
    if (rc) return rc;
    // fp16 far-plane guard.  The last sample of a ray has delta = 1e10 (volume_renderer.py:85-86): ANY sigma > 0 there makes alpha = 1, so
    // an fp16 rounding that flips the sign of a sigma within 1e-2 of zero turns a background ray into a full far-plane hit (round 2:
    // single rays off by 0.64 in rgb and 6.0 in depth, which alone set the fp16 PSNR).  Every other sample's alpha moves by
    // |d sigma| * delta ~ 1e-4.  So the fp16 precisions re-evaluate exactly that sample of every ray (0.5 % of the points) with the
    // split-fp16 stream that rides behind their packed model: fp32-accurate sigma and colour where it matters, ~1.5 % of the frame.
    const bool guard = fp16 && nb <= (int64_t)0x7fffffff / S;
    auto far_plane_guard = [&](const float* tvals, int64_t stride, int32_t S_, const void* packed_f16, float* raw) -> int {
      if (const int r2 = NERF_LAUNCH(nerf_last_sample_index_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), st, w.index, w.count,
                                     (long long)nb, S_)) return r2;
      return forward_rays(entry, o, d, tvals, stride, nb, S_, (const char*)packed_f16 + nerf::kF16PackedBytes, raw, false, nullptr, false,
                          false, NERF_PREC_F32X, stream, w.index, w.count);
    };
    if (n_importance == 0) {
      if (guard) {
        rc = far_plane_guard(tc, tcs, NERF_N_SAMPLES, packed_coarse, w.raw_c);
        if (rc) return rc;
      }
      rc = nerf_composite(w.raw_c, tc, tcs, nb, NERF_N_SAMPLES, white_bkgd, rgb_b, depth_b, nullptr, stream);
      if (rc) return rc;
      continue;
    }
    // fast_sampling, ESS/ERT (volume_renderer.py:359-369, network.py:207-253): the sampler also marks the valid merged samples
    rc = nerf_sample_fine_rays(w.raw_c, tc, tcs, u_rays ? u_rays + NERF_N_IMPORTANCE * r0 : u, u_rays ? NERF_N_IMPORTANCE : 0, nb, w.t_sorted,
                               nullptr, fast_sampling ? w.valid : nullptr, fast_sampling ? weights_threshold : 0.f, fast_sampling ? 0.45f : 0.f,
                               stream);
    if (rc) return rc;
    const bool cull_f = occ && occ->fine;
    if (cull_f) {
      rc = nerf_occupancy_mark(o, d, w.t_sorted, S, nb, (int32_t)S, occ->fine, occ->dims, occ->box_min, occ->inv_step, fast_sampling != 0, w.valid,
                               stream);
      if (rc) return rc;
    }
    if (!fast_sampling && !cull_f) {
      rc = forward_rays(entry, o, d, w.t_sorted, S, nb, (int32_t)S, packed_fine, w.raw_f, false, nullptr, false, true, precision, stream);
      if (rc) return rc;
      if (guard) {
        rc = far_plane_guard(w.t_sorted, S, (int32_t)S, packed_fine, w.raw_f);
        if (rc) return rc;
      }
    } else {
      // only the valid merged samples go through the fine network; the others keep raw = 0 (sigma 0 -> weight 0)
      rc = list_pass(w.valid, nb * S, w.index, w.raw_f);
      if (rc) return rc;
      rc = forward_rays(entry, o, d, w.t_sorted, S, nb, (int32_t)S, packed_fine, w.raw_f, false, nullptr, false, true, precision, stream,
                        w.index, w.count);
      if (rc) return rc;
    }
    rc = tally(1, fast_sampling || cull_f, nb * S);
    if (rc) return rc;
    // the guard of the masked fine pass.  Under fast_sampling alone the last merged sample of every ray is its coarse far sample,
    // and coarse samples are always valid: it is in the list, the fp16 network has just written it, and the exposure is the plain
    // branch's.  The list has been consumed (the forward and the tally are enqueued), so w.index / w.count are free for the guard's
    // ids.  With a fine occupancy field a last sample may be unlisted and must keep raw = 0: that combination stays as it is (the
    // package refuses fp16 with occupancy, modes.py).
    if (guard && fast_sampling && !cull_f) {
      rc = far_plane_guard(w.t_sorted, S, (int32_t)S, packed_fine, w.raw_f);
      if (rc) return rc;
    }
    rc = nerf_composite(w.raw_f, w.t_sorted, S, nb, (int32_t)S, white_bkgd, rgb_b, depth_b, nullptr, stream);
    if (rc) return rc;
  }
  return NERF_OK;
}

int32_t nerf_render_forward(const float* rays_o, const float* rays_d, int64_t n_rays,
                            const void* packed_coarse, const void* packed_fine,
                            const float* t_coarse, const float* u, int32_t n_importance,
                            int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                            float weights_threshold, void* workspace,
                            int64_t workspace_bytes, float* rgb, float* depth, void* stream) {
  return render_frame("nerf_render_forward", rays_o, rays_d, n_rays, packed_coarse, packed_fine, t_coarse, u, nullptr, nullptr, false,
                      n_importance, white_bkgd, precision, fast_sampling, weights_threshold, workspace, workspace_bytes, rgb, depth, stream);
}

int32_t nerf_render_forward_stochastic(const float* rays_o, const float* rays_d, int64_t n_rays,
                                       const void* packed_coarse, const void* packed_fine,
                                       const float* t_coarse, const float* u, const float* jitter, const float* u_rays,
                                       int32_t n_importance, int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                                       float weights_threshold, void* workspace, int64_t workspace_bytes,
                                       float* rgb, float* depth, void* stream) {
  if (precision != NERF_PREC_F32 && precision != NERF_PREC_F32X)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_render_forward_stochastic: precision must be f32 or f32x");
  if (fast_sampling) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_render_forward_stochastic: fast_sampling is not supported");
  return render_frame("nerf_render_forward_stochastic", rays_o, rays_d, n_rays, packed_coarse, packed_fine, t_coarse, u, jitter, u_rays,
                      true, n_importance, white_bkgd, precision, 0, weights_threshold, workspace, workspace_bytes, rgb, depth, stream);
}

}  // extern "C"

// ---- geometry out of a trained network: nerf_isosurface_* (kernels and entries)
#include "nerf_isosurface.hip.inc"
// ---- occupancy grid: nerf_occupancy_* and nerf_render_forward_occupancy
#include "nerf_occupancy.hip.inc"
// ---- geometry outputs: nerf_density_gradient and nerf_composite_normals
#include "nerf_normals.hip.inc"
// ---- mesh clean-up: nerf_mesh_components and nerf_mesh_filter_*
#include "nerf_mesh_components.hip.inc"
// ---- multiresolution hash-grid encoding: nerf_hashgrid_forward / nerf_hashgrid_backward
#include "nerf_hashgrid.hip.inc"
// ---- small fused ReLU MLP (include/nerf_mi355x_nn.h): nerf_fused_mlp_forward / nerf_fused_mlp_backward
#include "nerf_fused_mlp.hip.inc"
// ---- hash-grid radiance field, the ray-side glue (include/nerf_mi355x_nn.h): nerf_sh4_encode, nerf_field_*
#include "nerf_hashfield.hip.inc"
