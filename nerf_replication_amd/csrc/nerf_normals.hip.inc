// Geometry outputs: the density gradient at points (nerf_density_gradient) and the composited surface normal / opacity of a ray
// (nerf_composite_normals).  DESIGN.md section 2.10; the definitions are in include/nerf_mi355x.h.
// Needs, ahead of it, nerf_sampling.hip.inc (lane_bcast), nerf_composite.hip.inc (CompositeWeight, kCbMaxSamples), nerf_mlp_launch.hip.inc
// (forward_rays) and nerf_train_backward.hip.inc (backward_rays).
//
// No MLP kernel is added: a block of nerf_density_gradient is the density SAVE forward and the density chain (grads == NULL) of a
// training step, through their launchers.  The two kernels here are memory-trivial next to them (20 and 32 bytes per point against
// ~20 KB of saved / gradient rows).
#include "nerf_host.h"
#include "nerf_mlp_common.h"

namespace {

// raw [P,4] of the density SAVE forward -> the incoming gradient of the chain, draw [P,4] = (0, 0, 0, seed): seed = 1, or with
// positive_only [sigma > 0] (NaN: 0) -- then a 32-point tile without density is a dead tile of the backward pass.  Copies sigma out.
__global__ __launch_bounds__(256)
void nerf_density_seed_kernel(const float* __restrict__ raw, long long P, int positive_only, float* __restrict__ draw,
                              float* __restrict__ sigma_out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float s = raw[p * 4 + 3];
  const f32x4 seed = {0.f, 0.f, 0.f, (!positive_only || s > 0.0f) ? 1.0f : 0.0f};
  reinterpret_cast<f32x4*>(draw)[p] = seed;
  if (sigma_out) sigma_out[p] = s;
}

// acc = sum_k w_k, normal = sum_k w_k n_k with n_k = -g_k / |g_k| where sigma_k > 0 and g_k . g_k > 0, else 0.
// One wave per ray, four rays per workgroup.  Lane l owns samples l, l + 64, l + 128: it computes their CompositeWeight halves
// (alpha, q -- the expf) and their n_k in parallel, every load one coalesced row segment.  n_k is separately rounded fp32:
//     gg = fadd(fadd(fmul(gx, gx), fmul(gy, gy)), fmul(gz, gz));  r = sqrtf(gg);  n = __fdiv_rn(-g, r)
// both correctly rounded: sqrtf is v_sqrt_f32 plus the +-1 ulp residual correction (two v_fma_f32 and two selects; __fsqrt_rn
// would be the bare 1-ulp v_sqrt_f32), __fdiv_rn is v_div_scale / v_rcp / four v_fma / v_div_fmas / v_div_fixup -- the v_rcp_f32
// only seeds that IEEE sequence, there is no reciprocal or v_rsq shortcut.  Then ONE walk in sample order
// k = 0 .. S-1, the same in every lane (v_readlane of the owner's values): w_k = CompositeWeight::step, T carried as nerf_composite
// carries it, acc = fadd(acc, w_k), normal_c = fadd(normal_c, fmul(w_k, n_kc)).  So w_k is bit for bit nerf_composite's `weights`
// output, acc is the sum its kernels keep for the white background, and both sums run left to right over the samples.  No butterfly,
// no atomics: two runs write the same bytes.
__global__ __launch_bounds__(256)
void nerf_composite_normals_kernel(const float* __restrict__ raw, const float* __restrict__ tvals, long long t_ray_stride,
                                   long long n_rays, int S, const float* __restrict__ grad, float* __restrict__ normal_out,
                                   float* __restrict__ acc_out) {
  constexpr int C = kCbMaxSamples / 64;
  const int lane = threadIdx.x & 63;
  const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;                                   // (wave-uniform)
  const float* r1 = raw + ray * S * 4;
  const float* g3 = grad + ray * S * 3;
  const float* t = tvals + ray * t_ray_stride;
  CompositeWeight cw[C];
  float n[C][3];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int k = 64 * c + lane;
    const bool live = k < S;
    const float sigma = live ? r1[k * 4 + 3] : 0.0f;
    const float tk = live ? t[k] : 0.0f;
    const float tn = (k + 1 < S) ? t[k + 1] : tk;
    cw[c] = CompositeWeight::of(sigma, (k < S - 1) ? __fsub_rn(tn, tk) : 1e10f);
    const float gx = live ? g3[k * 3 + 0] : 0.0f, gy = live ? g3[k * 3 + 1] : 0.0f, gz = live ? g3[k * 3 + 2] : 0.0f;
    const float gg = __fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz));
    const float r = sqrtf(gg);
    const bool has = sigma > 0.0f && gg > 0.0f;                // (NaN: no normal)
    n[c][0] = has ? __fdiv_rn(-gx, r) : 0.0f;
    n[c][1] = has ? __fdiv_rn(-gy, r) : 0.0f;
    n[c][2] = has ? __fdiv_rn(-gz, r) : 0.0f;
  }
  float T = 1.0f, acc = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int m = S - 64 * c < 64 ? S - 64 * c : 64;           // samples of this chunk (wave-uniform; <= 0: none)
    for (int j = 0; j < m; ++j) {
      const CompositeWeight w = {lane_bcast(cw[c].alpha, j), lane_bcast(cw[c].q, j)};
      const float wk = w.step(T);
      acc = __fadd_rn(acc, wk);
      sx = __fadd_rn(sx, __fmul_rn(wk, lane_bcast(n[c][0], j)));
      sy = __fadd_rn(sy, __fmul_rn(wk, lane_bcast(n[c][1], j)));
      sz = __fadd_rn(sz, __fmul_rn(wk, lane_bcast(n[c][2], j)));
    }
  }
  if (lane == 0) {
    normal_out[ray * 3 + 0] = sx; normal_out[ray * 3 + 1] = sy; normal_out[ray * 3 + 2] = sz;
    acc_out[ray] = acc;
  }
}

// Bytes per point that nerf_density_gradient_point_bytes reports: the rows of TrainSave (2528 floats + 72 of sign bits) and
// TrainGrad (2432 floats), raw and draw (4 floats each) are 20 160 bytes; the rest covers the tile flags / list (8 bytes per 32
// points), the stamp and count words and the 256-byte alignment of the four pieces, for any whole number of 32-point tiles.
constexpr int64_t kDensityGradPointBytes = 20224;

// The workspace of one block of `pts` points, every piece 256-byte aligned
struct DensityGradWorkspace {
  float* save; float* gsave; float* raw; float* draw;
  int64_t bytes;
  DensityGradWorkspace(void* base, int64_t pts) {
    Carver c(base);
    save = c.take<float>(TrainSave::floats(pts));
    gsave = c.take<float>(TrainGrad::floats(pts));
    raw = c.take<float>(pts * 4);
    draw = c.take<float>(pts * 4);
    bytes = c.bytes();
  }
};
static_assert(32 * kDensityGradPointBytes >= 4 * (TrainSave::floats(32) + TrainGrad::floats(32) + 2 * 32 * 4) + 4 * 255 &&
              1024 * kDensityGradPointBytes >= 4 * (TrainSave::floats(1024) + TrainGrad::floats(1024) + 2 * 1024 * 4) + 4 * 255,
              "kDensityGradPointBytes must cover a block of whole tiles");

}  // namespace

extern "C" {

int64_t nerf_density_gradient_point_bytes(void) { return kDensityGradPointBytes; }

int32_t nerf_density_gradient(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                              int32_t n_samples, const void* packed, const void* packed_bwd, int32_t positive_only, float* sigma,
                              float* grad, int32_t precision, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* entry = "nerf_density_gradient";
  if (n_rays < 0 || n_samples <= 0 || n_samples > kCbMaxSamples || t_ray_stride < 0 || workspace_bytes < 0)
    return fail(NERF_ERR_INVALID_ARG, "%s: bad size (n_samples must be in 1..192)", entry);
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !tvals || !packed || !packed_bwd || !grad || !workspace)
    return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (precision != NERF_PREC_F32 && precision != NERF_PREC_F32X) return fail(NERF_ERR_UNSUPPORTED, "%s: f32 or f32x only", entry);
  // a block: as many whole rays as the workspace holds points (the reported bytes per point), checked against the exact layout
  int64_t B = workspace_bytes / kDensityGradPointBytes / n_samples;
  if (B > n_rays) B = n_rays;
  while (B > 0 && DensityGradWorkspace(nullptr, B * n_samples).bytes > workspace_bytes) --B;
  if (B <= 0) return fail(NERF_ERR_WORKSPACE, "%s: the workspace does not hold one ray", entry);
  hipStream_t st = (hipStream_t)stream;
  for (int64_t r0 = 0; r0 < n_rays; r0 += B) {
    const int64_t nb = n_rays - r0 < B ? n_rays - r0 : B;
    const int64_t P = nb * n_samples, p0 = r0 * n_samples;
    const float* o = rays_o + 3 * r0;
    const float* d = rays_d + 3 * r0;
    const float* t = tvals + r0 * t_ray_stride;
    const DensityGradWorkspace w(workspace, P);
    int rc = forward_rays(entry, o, d, t, t_ray_stride, nb, n_samples, packed, w.raw, true, w.save, true, false, precision, stream);
    if (rc) return rc;
    if ((rc = NERF_LAUNCH(nerf_density_seed_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), st, w.raw, (long long)P,
                          positive_only, w.draw, sigma ? sigma + p0 : nullptr))) return rc;
    rc = backward_rays(entry, o, d, t, t_ray_stride, nb, n_samples, packed_bwd, w.draw, w.save, w.gsave, nullptr, grad + 3 * p0, nullptr,
                       true, true, precision, stream);
    if (rc) return rc;
  }
  return NERF_OK;
}

int32_t nerf_composite_normals(const float* raw, const float* tvals, int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                               const float* grad, float* normal, float* acc, void* stream) {
  if (n_rays < 0 || n_samples <= 0 || t_ray_stride < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_normals: bad size");
  if (n_samples > kCbMaxSamples) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_normals: more than 192 samples per ray");
  if (n_rays == 0) return NERF_OK;
  if (!raw || !tvals || !grad || !normal || !acc) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_normals: null argument");
  const long long blocks = (n_rays + 3) / 4;
  if (blocks > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_composite_normals: too many rays for one launch");
  return NERF_LAUNCH(nerf_composite_normals_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, raw, tvals,
                     (long long)t_ray_stride, (long long)n_rays, n_samples, grad, normal, acc);
}

}  // extern "C"
