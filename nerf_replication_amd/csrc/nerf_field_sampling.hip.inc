// Where the samples of a hash-field ray lie (DESIGN.md section 2.14.2): importance sampling from the weights of a coarse pass,
// stratified jitter for any sample count, and the density-only scatter that feeds nerf_composite's `weights`.  The declarations and
// every formula are in include/nerf_mi355x_sampling.h.  fp32 throughout; the unit is compiled with -ffp-contract=off and every
// operation below is written with its own rounding, so each kernel is bit for bit the restatement in
// tests/hashfield_sampling_reference.py.  No atomics.
//
// Lane mappings:
//   sample_importance     one lane per ray, 64 rays per workgroup, modelled on nerf_sample_fine_kernel<true> (nerf_sampling.hip.inc):
//                         sequential sums in the header's order; every ray owns two padded LDS rows, staged and written back coalesced
//   stratified_depths     one thread per depth
//   density_scatter       one thread per row: one float4 store at the row's point id
#include "../../include/nerf_mi355x_sampling.h"
#include "nerf_host.h"

namespace {

constexpr int kFsThreads = 64;
constexpr int kFsMax = 192;          // Sc + Sf at most: nerf_composite's limit
constexpr int kFsPitch = 193;        // odd pitch: lanes walking their own rows never share a bank
constexpr int kFsTcPitch = 191;      // Sc <= 191 (Sf >= 1); odd as well

struct FieldSampleArgs {
  const float* weights;      // [n,Sc]
  const float* t_coarse;     // [Sc] or [n,Sc]
  long long t_stride;        // 0 or Sc
  const float* u;            // [Sf] or [n,Sf]
  long long u_stride;        // 0 or Sf
  long long n_rays;
  int Sc, Sf;
  float* t_merged;           // [n,Sc+Sf]
  float* t_fine;             // optional [n,Sf], in the caller's u order
};

// The inverse cdf at one u, given inds = #{cdf <= u}; cdf has K + 1 entries, tc has K + 2
__device__ __forceinline__ float fs_inv_cdf(const float* cdf, const float* tc, float u, int inds, int K) {
  const int below = min(max(inds - 1, 0), K), above = min(inds, K);
  const float cb = cdf[below], ca = cdf[above];
  const float bb = __fmul_rn(0.5f, __fadd_rn(tc[below + 1], tc[below]));
  const float ba = __fmul_rn(0.5f, __fadd_rn(tc[above + 1], tc[above]));
  float denom = __fsub_rn(ca, cb);
  if (denom < 1e-5f) denom = 1.0f;
  const float frac = __fdiv_rn(__fsub_rn(u, cb), denom);
  return __fadd_rn(bb, __fmul_rn(frac, __fsub_rn(ba, bb)));
}

// LDS per 64-ray workgroup: 64 x 193 + 64 x 191 floats = 98 304 B of the CU's 160 KiB: one workgroup (one wave) per CU.  The work is
// a chain of dependent LDS accesses per lane; a chunk of 16384 rays is 256 workgroups, one round of the device.
// A ray's row `buf`: slots [0, Sf) hold its u, then the sorted u, which the walk overwrites in place with the fine depths (slot
// j <= k is written only after u[k] was read); slots [Sf, Sf + K + 1) hold the interior weights, then the cdf; the merge from the
// back then fills all Sc + Sf slots (slot k is written when the unread fine depths lie in [0, jf], jf <= k, and the cdf is dead).
__global__ __launch_bounds__(kFsThreads)
void nerf_field_sample_importance_kernel(FieldSampleArgs a) {
  __shared__ float s_buf[kFsThreads * kFsPitch];
  __shared__ float s_tc[kFsThreads * kFsTcPitch];
  const int lane = threadIdx.x;
  const int Sc = a.Sc, Sf = a.Sf, K = Sc - 2, NB = K + 1, S = Sc + Sf;
  const long long ray0 = (long long)blockIdx.x * kFsThreads;
  for (int r = 0; r < kFsThreads; ++r) {               // coalesced: lane = position in the row
    long long rg = ray0 + r;
    if (rg >= a.n_rays) rg = a.n_rays - 1;             // a slot past the end recomputes the last ray and stores nothing
    const float* w = a.weights + rg * Sc;
    const float* t = a.t_coarse + rg * a.t_stride;
    const float* u = a.u + rg * a.u_stride;
    for (int i = lane; i < K; i += kFsThreads) s_buf[r * kFsPitch + Sf + i] = w[i + 1];
    for (int i = lane; i < Sc; i += kFsThreads) s_tc[r * kFsTcPitch + i] = t[i];
    for (int i = lane; i < Sf; i += kFsThreads) s_buf[r * kFsPitch + i] = u[i];
  }
  __syncthreads();
  float* buf = s_buf + lane * kFsPitch;
  float* cdf = buf + Sf;
  const float* tc = s_tc + lane * kFsTcPitch;

  // w' = w + eps in place, total left to right from w'_0; then cdf = [0, running sum of w' / total]
  float total = 0.0f;
  for (int i = 0; i < K; ++i) {
    const float we = __fadd_rn(cdf[i], 1e-5f);
    cdf[i] = we;
    total = i == 0 ? we : __fadd_rn(total, we);
  }
  {
    float run = 0.0f, prev = cdf[0];
    cdf[0] = 0.0f;
    for (int m = 1; m < NB; ++m) {
      run = __fadd_rn(run, __fdiv_rn(prev, total));
      if (m < K) prev = cdf[m];                        // (slot K holds no weight)
      cdf[m] = run;
    }
  }
  const long long ray = ray0 + lane;
  const bool ray_ok = ray < a.n_rays;
  if (a.t_fine && ray_ok) {                            // in the caller's order: the count by bisection (the cdf does not decrease)
    for (int k = 0; k < Sf; ++k) {
      const float u = buf[k];
      int lo = 0, hi = NB;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdf[mid] <= u) lo = mid + 1; else hi = mid; }
      a.t_fine[ray * Sf + k] = fs_inv_cdf(cdf, tc, u, lo, K);
    }
  }
  // the ray's u ascending: Shell sort in the lane's own row (gaps of Ciura); every index stays in [0, Sf)
  {
    const int gaps[6] = {132, 57, 23, 10, 4, 1};
#pragma unroll 1
    for (int g = 0; g < 6; ++g) {
      const int gap = gaps[g];
      for (int i = gap; i < Sf; ++i) {
        const float v = buf[i];
        int j = i;
        while (j >= gap && buf[j - gap] > v) { buf[j] = buf[j - gap]; j -= gap; }
        buf[j] = v;
      }
    }
  }
  // inverse cdf at the ascending u: the count only grows
  int ind = 0;
  for (int k = 0; k < Sf; ++k) {
    const float u = buf[k];
    while (ind < NB && cdf[ind] <= u) ++ind;
    const float v = fs_inv_cdf(cdf, tc, u, ind, K);
    int j = k;                                         // keeps the fine depths ascending whatever rounding does
    while (j > 0 && buf[j - 1] > v) { buf[j] = buf[j - 1]; --j; }
    buf[j] = v;
  }
  // two-way merge from the back of (coarse depths, fine depths)
  {
    int ic = Sc - 1, jf = Sf - 1;
    for (int k = S - 1; k >= 0; --k) {
      const bool take_f = (ic < 0) || (jf >= 0 && buf[jf] >= tc[ic]);
      if (take_f) { buf[k] = buf[jf]; --jf; }
      else { buf[k] = tc[ic]; --ic; }
    }
  }
  __syncthreads();
  for (int r = 0; r < kFsThreads; ++r) {               // coalesced: lane = position in the row
    const long long rg = ray0 + r;
    if (rg >= a.n_rays) break;
    for (int k = lane; k < S; k += kFsThreads) a.t_merged[rg * S + k] = s_buf[r * kFsPitch + k];
  }
}

__global__ __launch_bounds__(256)
void nerf_field_stratified_kernel(const float* __restrict__ t_tab, const float* __restrict__ jitter, long long n_elems, int S,
                                  float* __restrict__ t_out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_elems) return;
  const int s = (int)(e % S);
  const float lower = s == 0 ? t_tab[0] : __fmul_rn(0.5f, __fadd_rn(t_tab[s], t_tab[s - 1]));
  const float upper = s == S - 1 ? t_tab[S - 1] : __fmul_rn(0.5f, __fadd_rn(t_tab[s + 1], t_tab[s]));
  t_out[e] = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), jitter[e]));
}

__global__ __launch_bounds__(256)
void nerf_field_density_scatter_kernel(const float* __restrict__ sigma, long long sigma_stride, const int* __restrict__ index,
                                       uint32_t n_rows, uint32_t n_points, float* __restrict__ raw) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_rows) return;
  const uint32_t id = index ? (uint32_t)index[j] : j;
  if (id >= n_points) return;
  reinterpret_cast<float4*>(raw)[id] = make_float4(0.f, 0.f, 0.f, sigma[(long long)j * sigma_stride]);
}

bool fs_misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

}  // namespace

extern "C" {

int32_t nerf_field_sample_importance(const float* weights, const float* t_coarse, int64_t t_ray_stride, const float* u,
                                     int64_t u_ray_stride, int64_t n_rays, int32_t n_coarse, int32_t n_fine, float* t_merged,
                                     float* t_fine, void* stream) {
  const char* entry = "nerf_field_sample_importance";
  if (n_coarse < 3 || n_fine < 1 || (int64_t)n_coarse + n_fine > kFsMax)
    return fail(NERF_ERR_INVALID_ARG, "%s: needs n_coarse >= 3, n_fine >= 1 and n_coarse + n_fine <= 192", entry);
  if (n_rays <= 0 || n_rays > 0x7fffffffLL / (n_coarse + n_fine))
    return fail(NERF_ERR_INVALID_ARG, "%s: n_rays must be positive and n_rays * (n_coarse + n_fine) at most 2^31 - 1", entry);
  if ((t_ray_stride != 0 && t_ray_stride != n_coarse) || (u_ray_stride != 0 && u_ray_stride != n_fine))
    return fail(NERF_ERR_INVALID_ARG, "%s: a ray stride is 0 or the row length (t: n_coarse, u: n_fine)", entry);
  if (!weights || !t_coarse || !u || !t_merged) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (fs_misaligned(weights, 4) || fs_misaligned(t_coarse, 4) || fs_misaligned(u, 4) || fs_misaligned(t_merged, 4) ||
      fs_misaligned(t_fine, 4))
    return fail(NERF_ERR_INVALID_ARG, "%s: every pointer must be aligned to 4 bytes", entry);
  FieldSampleArgs a;
  a.weights = weights; a.t_coarse = t_coarse; a.t_stride = t_ray_stride; a.u = u; a.u_stride = u_ray_stride; a.n_rays = n_rays;
  a.Sc = n_coarse; a.Sf = n_fine; a.t_merged = t_merged; a.t_fine = t_fine;
  return NERF_LAUNCH(nerf_field_sample_importance_kernel, dim3((unsigned)((n_rays + kFsThreads - 1) / kFsThreads)), dim3(kFsThreads),
                     (hipStream_t)stream, a);
}

int32_t nerf_field_stratified_depths(const float* t_table, const float* jitter, int64_t n_rays, int32_t n_samples, float* t,
                                     void* stream) {
  const char* entry = "nerf_field_stratified_depths";
  if (n_samples < 1 || n_samples > kFsMax) return fail(NERF_ERR_INVALID_ARG, "%s: n_samples must be in [1, 192]", entry);
  if (n_rays <= 0 || n_rays > 0x7fffffffLL / n_samples)
    return fail(NERF_ERR_INVALID_ARG, "%s: n_rays must be positive and n_rays * n_samples at most 2^31 - 1", entry);
  if (!t_table || !jitter || !t) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (fs_misaligned(t_table, 4) || fs_misaligned(jitter, 4) || fs_misaligned(t, 4))
    return fail(NERF_ERR_INVALID_ARG, "%s: every pointer must be aligned to 4 bytes", entry);
  const long long ne = (long long)n_rays * n_samples;
  return NERF_LAUNCH(nerf_field_stratified_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), (hipStream_t)stream, t_table, jitter,
                     ne, (int)n_samples, t);
}

int32_t nerf_field_density_scatter(const float* sigma, int64_t sigma_stride, const int32_t* index, int64_t n_rows, int64_t n_points,
                                   float* raw, void* stream) {
  const char* entry = "nerf_field_density_scatter";
  if (n_points <= 0 || n_points > 0x7fffffffLL || n_rows <= 0 || n_rows > n_points)
    return fail(NERF_ERR_INVALID_ARG, "%s: needs 1 <= n_rows <= n_points <= 2^31 - 1", entry);
  if (sigma_stride < 1) return fail(NERF_ERR_INVALID_ARG, "%s: sigma_stride must be at least 1", entry);
  if (!sigma || !raw) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (fs_misaligned(sigma, 4) || fs_misaligned(index, 4) || fs_misaligned(raw, 16))
    return fail(NERF_ERR_INVALID_ARG, "%s: sigma and index must be aligned to 4 bytes, raw to 16", entry);
  return NERF_LAUNCH(nerf_field_density_scatter_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), (hipStream_t)stream, sigma,
                     (long long)sigma_stride, index, (uint32_t)n_rows, (uint32_t)n_points, raw);
}

}  // extern "C"
