// Packed weight streams (nerf_layout.h): the pack kernels of every precision, the fold of feature_linear into the views layer, the
// transposed streams of the backward chain, and their entries nerf_pack_model / nerf_pack_model_ordered / nerf_pack_model_bwd /
// nerf_packed_*_bytes.
#include "../../include/nerf_mi355x_order.h"
#include "nerf_host.h"
#include "nerf_mlp_common.h"

namespace {

// ------------------------------------------------------------------------------------ pack
struct PackArgs {
  const float* p[nerf::P_COUNT];
  float* out;
};

// Unit orders (include/nerf_mi355x_order.h): order[l][position] = the original unit of h_l at `position` of the permuted network,
// whose stream the fp32 pack kernel writes; a null table is the identity (every other pack kernel passes none).
__device__ __forceinline__ int ordered_unit(const uint8_t* order, int l, int position) {
  return order ? (int)order[l * nerf::kHidden + position] : position;
}

__device__ __forceinline__ float pack_weight_elem(const PackArgs& a, long long rel, int ntiles,
                                                  int which /*0 L0,1 hidden,2 L5a,3 L5b,4 feat,5 views*/,
                                                  int layer, const uint8_t* order) {
  using namespace nerf;
  const int q = (int)(rel & 3);
  const int lane = (int)((rel >> 2) & 63);
  const long long blk = rel >> 8;                 // g*NT + j
  const int j = (int)(blk % ntiles);
  const int g = (int)(blk / ntiles);
  const int s = 4 * g + q, t = s >> 4, r = s & 15, h = lane >> 5;
  const int out = 32 * j + (lane & 31);
  switch (which) {
    case 0: { const int c = pe_xyz_feat(s, h); return c < 0 ? 0.f : a.p[P_W0][ordered_unit(order, 0, out) * 63 + c]; }
    case 1: return a.p[2 * layer][ordered_unit(order, layer, out) * 256 + ordered_unit(order, layer - 1, act_feat(t, r, h))];
    case 2: { const int c = pe_xyz_feat(s, h); return c < 0 ? 0.f : a.p[10][ordered_unit(order, 5, out) * 319 + c]; }
    case 3: return a.p[10][ordered_unit(order, 5, out) * 319 + 63 + ordered_unit(order, 4, act_feat(t, r, h))];
    case 4: return a.p[P_WF][out * 256 + ordered_unit(order, 7, act_feat(t, r, h))];
    default: {                                      // (its inputs are feature_linear's outputs and the direction: not permuted)
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
// the same over the units of h_l in `order` (the fp32 pack kernel alone: the other kernels' helpers stay as they were)
template <int LOG2>
__device__ __forceinline__ float act_order_value_ordered(const float* x, int rel, const uint8_t* order, int l) {
  const int h = rel >> LOG2, slot = rel & ((1 << LOG2) - 1);
  return x[ordered_unit(order, l, nerf::act_feat(slot >> 4, slot & 15, h))];
}
// The blocks the streams share beside w_alpha (act_order_value<7>): biases [layer 0..8][h][j*16 + r], w_rgb [c][h][t*16 + r] (t < 4)
// and the head biases b_rgb[3], b_alpha.  (The weight pointer, not PackArgs, where a kernel also picks a weight matrix by a
// run-time index: a reference to the arguments there made the compiler copy them to scratch.)
__device__ __forceinline__ float pack_bias_value(const PackArgs& a, int rel) {
  const int layer = rel >> 8;
  return act_order_value<7>(layer < 8 ? a.p[2 * layer + 1] : a.p[nerf::P_BF], rel & 255);
}
__device__ __forceinline__ float pack_bias_value_ordered(const PackArgs& a, int rel, const uint8_t* order) {
  const int layer = rel >> 8;                     // (feature_linear's outputs, layer 8, are not permuted)
  return layer < 8 ? act_order_value_ordered<7>(a.p[2 * layer + 1], rel & 255, order, layer) : act_order_value<7>(a.p[nerf::P_BF], rel & 255);
}
__device__ __forceinline__ float pack_w_rgb_value(const float* w_rgb, int rel) {
  return act_order_value<6>(w_rgb + 128 * (rel >> 7), rel & 127);
}
__device__ __forceinline__ float pack_head_bias_value(const PackArgs& a, int rel) {
  return rel < 3 ? a.p[nerf::P_BR][rel] : a.p[nerf::P_BA][0];
}

__global__ void nerf_pack_kernel(PackArgs a, const uint8_t* __restrict__ order) {
  using namespace nerf;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kUnfoldedFloats) return;
  constexpr long long WS = wsize(128, 8);
  float v;
  if (i < kOffL1) v = pack_weight_elem(a, i - kOffL0, 8, 0, 0, order);
  else if (i < kOffL5a) { const long long rel = i - kOffL1; v = pack_weight_elem(a, rel % WS, 8, 1, 1 + (int)(rel / WS), order); }
  else if (i < kOffL5b) v = pack_weight_elem(a, i - kOffL5a, 8, 2, 5, order);
  else if (i < kOffL6) v = pack_weight_elem(a, i - kOffL5b, 8, 3, 5, order);
  else if (i < kOffFeat) { const long long rel = i - kOffL6; v = pack_weight_elem(a, rel % WS, 8, 1, 6 + (int)(rel / WS), order); }
  else if (i < kOffViews) v = pack_weight_elem(a, i - kOffFeat, 8, 4, 0, order);
  else if (i < kOffBias) v = pack_weight_elem(a, i - kOffViews, 4, 5, 0, order);
  else if (i < kOffBiasViews) v = pack_bias_value_ordered(a, (int)(i - kOffBias), order);
  else if (i < kOffWAlpha) v = act_order_value<6>(a.p[P_BV], (int)(i - kOffBiasViews));      // [h][j*16 + r], j < 4
  else if (i < kOffWRgb) v = act_order_value_ordered<7>(a.p[P_WA], (int)(i - kOffWAlpha), order, 7);
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

}  // namespace

extern "C" {

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

// the fp32 stream: the permuted parameters (order: device [8][256] or null = identity), then the fold computed from them
static int32_t pack_f32(const PackArgs& a, const uint8_t* order, hipStream_t st) {
  const unsigned blocks = (unsigned)((nerf::kUnfoldedFloats + 255) / 256);
  if (const int rc = NERF_LAUNCH(nerf_pack_kernel, dim3(blocks), dim3(256), st, a, order)) return rc;
  return NERF_LAUNCH(nerf_fold_f32_kernel, dim3(kFoldBlocks), dim3(256), st, (const float*)a.out, a.out + nerf::kOffFold);
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
  return pack_f32(a, nullptr, (hipStream_t)stream);
}

// include/nerf_mi355x_order.h: the fp32 stream of the network permuted by `order` (null: nerf_pack_model's bytes)
int32_t nerf_pack_model_ordered(const float* const params[24], const uint8_t* order, void* packed, int32_t precision, void* stream) {
  PackArgs a;
  if (const int rc = fill_pack_args("nerf_pack_model_ordered", params, packed, a)) return rc;
  if (precision != NERF_PREC_F32) return fail(NERF_ERR_UNSUPPORTED, "%s", "nerf_pack_model_ordered: f32 only");
  return pack_f32(a, order, (hipStream_t)stream);
}

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

}  // extern "C"
