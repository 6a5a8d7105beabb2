// Volume compositing of the samples of a ray (volume_renderer.py:67-96, :414-432): the two forward kernels, the adjoint, and the
// entries nerf_composite / nerf_composite_backward.
// Needs nerf_sampling.hip.inc ahead of it (alpha_of, wave_scan / wave_shift and their ops).
#include "nerf_host.h"
#include "nerf_mlp_common.h"

namespace {

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
// load and store is one coalesced row segment.
constexpr int kCbMaxSamples = 192;

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
  const double wb = white_bkgd ? 1.0 : 0.0;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // The discrete decisions -- the relu mask and whether clamp(1 - alpha, 1e-10, 1) passes the gradient -- are the forward's: fp32,
  // its expf, its rounding.  Everything smooth is float64 from the inputs (exp included): in fp32, 1 - alpha sits on a grid of
  // 2^-24, so behind a nearly opaque sample q = e carries a relative error of 2^-25 / e, and the difference g_w T - suf / q then
  // lands as far from a float64 evaluation as the accident of that rounding decides (tests/test_gpu_ray_side.py measured 0.3 to 7
  // times the distance of an fp32 evaluation on the CPU, on rays with an opaque sample).  The adjoint is 4096 waves of a training
  // step; the twelve double-precision exp per lane do not show in the step time.
  f32x4 v[C];
  float tk[C];
  bool pass[C];
  double delta[C], e[C], alpha[C], q[C], Tk[C], g_delta[C], gt_own[C];
  // forward sweep: T_k = prod_{j<k} q_j
  double carry = 1.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int k = 64 * c + lane;
    const bool live = k < S;
    v[c] = live ? r4[k] : zero4;
    tk[c] = live ? t[k] : 0.0f;
    const float tn = (k + 1 < S) ? t[k + 1] : tk[c];
    const float sig = fmaxf(v[c].w, 0.0f);
    const float delta32 = (k < S - 1) ? __fsub_rn(tn, tk[c]) : 1e10f;
    const float om32 = __fsub_rn(1.0f, alpha_of(sig, delta32));             // the forward's 1 - alpha
    pass[c] = om32 >= 1e-10f && om32 <= 1.0f;
    delta[c] = (k < S - 1) ? (double)tn - (double)tk[c] : 1e10;
    e[c] = exp(-(double)sig * delta[c]);
    alpha[c] = 1.0 - e[c];
    const double om = 1.0 - alpha[c];
    q[c] = !live ? 1.0 : pass[c] ? om : fmin(fmax(om, 1e-10), 1.0);
    const double p = wave_scan<true>(q[c], lane, op_prod);
    Tk[c] = carry * wave_shift<true>(p, lane, 1.0);
    carry *= __shfl(p, 63);
  }
  // reverse sweep: suf_k = sum_{m>k} g_w_m a_m T_m;  g_q_k = suf_k / q_k
  auto sigmoid64 = [](float x) { return 1.0 / (1.0 + exp(-(double)x)); };
  double carry_s = 0.0;
#pragma unroll
  for (int c = C - 1; c >= 0; --c) {
    const int k = 64 * c + lane;
    const bool live = k < S;
    const double sig = (double)fmaxf(v[c].w, 0.0f);
    const double cr = sigmoid64(v[c].x), cg = sigmoid64(v[c].y), cb = sigmoid64(v[c].z);
    const double g_w = (double)gr * (cr - wb) + (double)gg * (cg - wb) + (double)gb * (cb - wb) + (double)gd * (double)tk[c];
    const double w = Tk[c] * alpha[c];
    const double sfx = wave_scan<false>(live ? g_w * alpha[c] * Tk[c] : 0.0, lane, op_sum);
    const double suf = wave_shift<false>(sfx, lane, 0.0) + carry_s;
    carry_s += __shfl(sfx, 0);
    double g_alpha = g_w * Tk[c];
    if (pass[c]) g_alpha -= suf / q[c];                          // clamp passes the gradient inside its range
    const double g_sig = g_alpha * delta[c] * e[c];
    g_delta[c] = (k < S - 1) ? g_alpha * sig * e[c] : 0.0;
    f32x4 go;
    go.x = (float)((double)gr * w * cr * (1.0 - cr));
    go.y = (float)((double)gg * w * cg * (1.0 - cg));
    go.z = (float)((double)gb * w * cb * (1.0 - cb));
    go.w = v[c].w > 0.0f ? (float)g_sig : 0.0f;
    if (live) g4[k] = go;
    gt_own[c] = (double)gd * w - g_delta[c];                     // delta_k = t_{k+1} - t_k: - g_delta_k here, + g_delta_{k-1} below
  }
  if (gt) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int k = 64 * c + lane;
      const double last_of_prev_chunk = c > 0 ? __shfl(g_delta[c > 0 ? c - 1 : 0], 63) : 0.0;
      if (k < S) gt[k] = (float)(gt_own[c] + wave_shift<true>(g_delta[c], lane, last_of_prev_chunk));
    }
  }
}

}  // namespace

extern "C" {

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

}  // extern "C"
