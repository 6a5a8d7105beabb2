// The backward pass of a training step behind the compositing and sampling adjoints: live-tile lists, the masked (compact-row) pass,
// the ray adjoints, the weight-gradient launches (nerf_wgrad_table.h), the data-gradient chain with everything around it
// (mlp_backward_impl), their entries, and the fused clip + Adam step.
// Needs, ahead of it, the backward and weight-gradient kernel files (nerf_mlp_bwd_f32 / bwd_f32x / wgrad_f32 / wgrad_bf16x3.hip.inc)
// and nerf_mlp_launch.hip.inc (dead_tile_list_available, persistent_blocks, masked_sizes_ok).
#include "nerf_host.h"
#include "nerf_mlp_common.h"
#include "nerf_wgrad_table.h"
#include "nerf_scan.hip.inc"

namespace {

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
// The rays adjoint (DESIGN section 2, "Gradients with respect to the rays").  Ray mode: the fine pass encodes v = d / |d|, rounded
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

// A dense backward on a save buffer whose forward skipped rows (TrainSave::off_stamp, dead_tile_list_available): poison
__global__ void nerf_check_stamp_kernel(const float* __restrict__ stamp, float* __restrict__ poison) {
  if (threadIdx.x == 0 && __float_as_int(stamp[0]) != 0) poison[0] = __int_as_float(0x7fc00000);
}

// ------------------------------------------------------------------------------------ fused clip + Adam (section 8f-4)
// One launch over all 48 parameter tensors: clip_grad_value_ (trainer.py:59) + torch.optim.Adam's update
// (optimizer.py:21-24: Adam(lr, weight_decay, eps), betas (0.9, 0.999), no amsgrad) in the operation order of torch's
// device kernels, every operation rounded on its own:
//     g = clamp(g, -clip, clip)  (NaN stays NaN, +-inf becomes +-clip);   g = g + wd * p  (wd != 0)
//     m = m + (g - m) * w1  (w1 < 0.5)   or   g - (g - m) * (1 - w1)  (w1 >= 0.5: the two forms of torch's lerp)
//     v = v * b2 + (g * g) * w2;   denom = sqrt(v) / bc2s + eps;   p = p + s * (m / denom)
// The constants are formed in double on the host, as torch forms them from Python floats, and rounded to fp32 once:
//     w1 = 1 - beta1, b2 = beta2, w2 = 1 - beta2, bc2s = sqrt(1 - beta2^step), s = -(lr / (1 - beta1^step)).
// sqrtf and __fdiv_rn are the correctly rounded forms here (__fsqrt_rn would be the bare 1-ulp v_sqrt_f32, nerf_normals.hip.inc);
// tests/adam_reference.py restates the step and tests/test_gpu_adam.py holds the kernel to it bit for bit.
constexpr int kAdamMaxTensors = 48;
struct AdamArgs {
  float* p[kAdamMaxTensors];
  const float* g[kAdamMaxTensors];
  float* m[kAdamMaxTensors];
  float* v[kAdamMaxTensors];
  long long end[kAdamMaxTensors];      // exclusive prefix ends of the flattened index space (a zero-element tensor repeats its
  int n_tensors;                       // predecessor's end: the search below never lands on it)
  float w1, b2, w2, bc2s, s, eps, weight_decay, clip;
};
__global__ __launch_bounds__(256)
void nerf_adam_kernel(AdamArgs a) {
  const long long total = a.end[a.n_tensors - 1];
  const float w1c = __fsub_rn(1.0f, a.w1);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = a.n_tensors - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (i < a.end[mid]) hi = mid; else lo = mid + 1; }
    const long long j = i - (lo ? a.end[lo - 1] : 0);
    float g = a.g[lo][j];
    if (a.clip > 0.0f) { if (g < -a.clip) g = -a.clip; if (g > a.clip) g = a.clip; }     // two comparisons: NaN passes, as clamp_
    const float p = a.p[lo][j];
    if (a.weight_decay != 0.0f) g = __fadd_rn(g, __fmul_rn(a.weight_decay, p));
    float m = a.m[lo][j], v = a.v[lo][j];
    const float d = __fsub_rn(g, m);                                                    // exp_avg.lerp_(grad, 1 - beta1)
    m = a.w1 < 0.5f ? __fadd_rn(m, __fmul_rn(d, a.w1)) : __fsub_rn(g, __fmul_rn(d, w1c));
    v = __fadd_rn(__fmul_rn(v, a.b2), __fmul_rn(__fmul_rn(g, g), a.w2));                // mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), a.bc2s), a.eps);
    a.m[lo][j] = m; a.v[lo][j] = v;
    a.p[lo][j] = __fadd_rn(p, __fmul_rn(a.s, __fdiv_rn(m, denom)));                     // addcdiv_(m, denom, value=-step_size)
  }
}

}  // namespace

extern "C" {

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

int64_t nerf_train_grad_floats(int64_t n_points) { return n_points < 0 ? -1 : TrainGrad::floats(n_points); }
int64_t nerf_train_live_count_offset(int64_t n_points) { return n_points < 0 ? -1 : TrainGrad::off_count(n_points); }

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

int32_t nerf_adam_step(int32_t n_tensors, float* const params[], const float* const grads[], float* const exp_avg[],
                       float* const exp_avg_sq[], const int64_t numel[], double lr, double beta1, double beta2, double eps,
                       double weight_decay, double clip_value, int64_t step, void* stream) {
  if (n_tensors <= 0 || n_tensors > kAdamMaxTensors || step <= 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: bad size");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: null argument");
  AdamArgs a;
  long long run = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (numel[i] < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: bad size");
    // a zero-element tensor (an empty device tensor has a null data pointer) is stepped over: its pointers are not examined
    if (numel[i] > 0 && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i])) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_adam_step: null tensor");
    a.p[i] = params[i]; a.g[i] = grads[i]; a.m[i] = exp_avg[i]; a.v[i] = exp_avg_sq[i];
    run += numel[i]; a.end[i] = run;
  }
  if (run == 0) return NERF_OK;
  // the constants as torch.optim.Adam forms them: in double from the double hyper-parameters, each rounded to fp32 once
  a.n_tensors = n_tensors;
  a.w1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.w2 = (float)(1.0 - beta2);
  a.bc2s = (float)sqrt(1.0 - pow(beta2, (double)step));
  a.s = (float)-(lr / (1.0 - pow(beta1, (double)step)));
  a.eps = (float)eps; a.weight_decay = (float)weight_decay; a.clip = (float)clip_value;
  long long blocks = (run + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  return NERF_LAUNCH(nerf_adam_kernel, dim3((unsigned)blocks), dim3(256), (hipStream_t)stream, a);
}

}  // extern "C"
