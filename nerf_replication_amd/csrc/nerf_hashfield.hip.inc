// Ray-side glue of the hash-grid radiance field (DESIGN.md section 2.14): what sits between nerf_occupancy_mark / nerf_compact_valid,
// nerf_hashgrid_forward, nerf_fused_mlp_forward and nerf_composite.  The declarations and every formula are in
// include/nerf_mi355x_nn.h.  fp32 throughout; the unit is compiled with -ffp-contract=off and every operation below is written with its own rounding, so each kernel is bit for bit the fp32 restatement in
// tests/hashfield_reference.py.  Memory-bound copies and a few flops per row: 256 threads, no LDS, no atomics; rows are indexed with
// 32 bits (the entries refuse more than 2^31 - 1 point ids), addresses are formed in 64 bits.
//
// Lane mappings:
//   sh4_encode              one thread per ray: 3 loads, 16 values as four float4 stores
//   field_points            one thread per row: the id, o + d t, clamp, normalise; three plain stores (rows of 12 bytes)
//   field_color_inputs      one thread per float4 of a cin row (8 per row): 0..3 copy the geometry feature, 4..7 the ray's SH block;
//                           thread 0 of a row also stores the row's sigma (geo column 0)
//   color_inputs_backward   one thread per float4 of a g_geo row (4 per row)
//   raw_scatter / gather    one thread per row: one float4 store / load at the row's point id; an id outside [0, n_points) is
//                           skipped (the scatter) or read as zero (the gather), so no index reaches outside `raw`

#include "../../include/nerf_mi355x_nn.h"
#include "nerf_host.h"
#include "../../include/nerf_mi355x_field.h"      // the spatial adjoint of the same glue: the kernels behind "the spatial adjoint" below

namespace {

constexpr int kHfBlock = 256;
constexpr int kHfMaxSamples = 192;
constexpr int kHfGeo = 16;               // geometry-feature columns = SH coefficients per ray; a cin row is both, 32 floats

struct HfBox {                           // passed by value in the kernel arguments
  float lo[3], hi[3];
};

__global__ __launch_bounds__(kHfBlock)
void nerf_sh4_encode_kernel(const float* __restrict__ rays_d, uint32_t n_rays, float* __restrict__ sh) {
  const uint32_t r = blockIdx.x * kHfBlock + threadIdx.x;
  if (r >= n_rays) return;
  const float* __restrict__ d = rays_d + (size_t)r * 3;
  float x = d[0], y = d[1], z = d[2];
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
  const float nrm = sqrtf(s);                                  // correctly rounded (__fsqrt_rn is the native, approximate one here)
  x = __fdiv_rn(x, nrm); y = __fdiv_rn(y, nrm); z = __fdiv_rn(z, nrm);
  const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y);
  const float xmy = __fsub_rn(xx, yy);                                        // x*x - y*y
  const float z5 = __fmul_rn(__fmul_rn(5.0f, z), z);                          // 5*z*z
  const float om5 = __fsub_rn(1.0f, z5);                                      // 1 - 5*z*z
  float4* __restrict__ out = reinterpret_cast<float4*>(sh + (size_t)r * kHfGeo);
  out[0] = make_float4(0.28209479177387814f,
                       __fmul_rn(-0.48860251190291987f, y),
                       __fmul_rn(0.48860251190291987f, z),
                       __fmul_rn(-0.48860251190291987f, x));
  out[1] = make_float4(__fmul_rn(__fmul_rn(1.0925484305920792f, x), y),
                       __fmul_rn(__fmul_rn(-1.0925484305920792f, y), z),
                       __fsub_rn(__fmul_rn(__fmul_rn(0.94617469575755997f, z), z), 0.31539156525251999f),
                       __fmul_rn(__fmul_rn(-1.0925484305920792f, x), z));
  out[2] = make_float4(__fmul_rn(0.54627421529603959f, xmy),
                       __fmul_rn(__fmul_rn(0.59004358992664352f, y), __fadd_rn(__fmul_rn(__fmul_rn(-3.0f, x), x), yy)),
                       __fmul_rn(__fmul_rn(__fmul_rn(2.8906114426405538f, x), y), z),
                       __fmul_rn(__fmul_rn(0.45704579946446572f, y), om5));
  out[3] = make_float4(__fmul_rn(__fmul_rn(0.3731763325901154f, z), __fsub_rn(z5, 3.0f)),
                       __fmul_rn(__fmul_rn(0.45704579946446572f, x), om5),
                       __fmul_rn(__fmul_rn(1.4453057213202769f, z), xmy),
                       __fmul_rn(__fmul_rn(0.59004358992664352f, x), __fadd_rn(__fmul_rn(-x, x), __fmul_rn(__fmul_rn(3.0f, y), y))));
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_points_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ tvals,
                              long long t_ray_stride, uint32_t n_samples, const int* __restrict__ index, uint32_t n_rows,
                              uint32_t n_points, HfBox box, float extent, float* __restrict__ x) {
  const uint32_t j = blockIdx.x * kHfBlock + threadIdx.x;
  if (j >= n_rows) return;
  uint32_t id = index ? (uint32_t)index[j] : j;
  if (id >= n_points) id = n_points - 1;                       // a read only; a list from nerf_compact_valid never gets here
  const uint32_t ray = id / n_samples, s = id - ray * n_samples;
  const float* __restrict__ o = rays_o + (size_t)ray * 3;
  float p[3] = {o[0], o[1], o[2]};
  if (rays_d) {                                                // (NULL: point mode, the entry has checked n_samples == 1)
    const float* __restrict__ d = rays_d + (size_t)ray * 3;
    const float t = tvals[(long long)ray * t_ray_stride + s];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fadd_rn(p[a], __fmul_rn(d[a], t));      // nerf_occupancy_mark's two roundings
  }
  float* __restrict__ out = x + (size_t)j * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = fminf(fmaxf(p[a], box.lo[a]), box.hi[a]);
    out[a] = __fdiv_rn(__fsub_rn(c, box.lo[a]), extent);
  }
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_color_inputs_kernel(const float* __restrict__ geo, const float* __restrict__ sh, const int* __restrict__ index,
                                    uint32_t n_rows, uint32_t n_samples, uint32_t n_points, float* __restrict__ cin,
                                    float* __restrict__ sigma_rows) {
  const unsigned long long t = (unsigned long long)blockIdx.x * kHfBlock + threadIdx.x;
  const uint32_t q = (uint32_t)(t & 7u);
  if ((t >> 3) >= n_rows) return;
  const uint32_t j = (uint32_t)(t >> 3);
  float4 v;
  if (q < 4) {
    v = reinterpret_cast<const float4*>(geo + (size_t)j * kHfGeo)[q];
    if (q == 0) sigma_rows[j] = v.x;
  } else {
    uint32_t id = index ? (uint32_t)index[j] : j;
    if (id >= n_points) id = n_points - 1;                     // a read only, as in nerf_field_points_kernel
    v = reinterpret_cast<const float4*>(sh + (size_t)(id / n_samples) * kHfGeo)[q - 4];
  }
  reinterpret_cast<float4*>(cin + (size_t)j * (2 * kHfGeo))[q] = v;
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_color_inputs_backward_kernel(const float* __restrict__ g_cin, const float* __restrict__ g_sigma_rows, uint32_t n_rows,
                                             float* __restrict__ g_geo) {
  const unsigned long long t = (unsigned long long)blockIdx.x * kHfBlock + threadIdx.x;
  const uint32_t q = (uint32_t)(t & 3u);
  if ((t >> 2) >= n_rows) return;
  const uint32_t j = (uint32_t)(t >> 2);
  float4 v = reinterpret_cast<const float4*>(g_cin + (size_t)j * (2 * kHfGeo))[q];
  if (q == 0) v.x = __fadd_rn(v.x, g_sigma_rows[j]);
  reinterpret_cast<float4*>(g_geo + (size_t)j * kHfGeo)[q] = v;
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_raw_scatter_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma_rows, const int* __restrict__ index,
                                   uint32_t n_rows, uint32_t n_points, float* __restrict__ raw) {
  const uint32_t j = blockIdx.x * kHfBlock + threadIdx.x;
  if (j >= n_rows) return;
  const uint32_t id = index ? (uint32_t)index[j] : j;
  if (id >= n_points) return;
  const float* __restrict__ c = rgb + (size_t)j * 3;
  reinterpret_cast<float4*>(raw)[id] = make_float4(c[0], c[1], c[2], sigma_rows[j]);
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_raw_gather_kernel(const float* __restrict__ g_raw, const int* __restrict__ index, uint32_t n_rows, uint32_t n_points,
                                  float* __restrict__ g_rgb, float* __restrict__ g_sigma_rows) {
  const uint32_t j = blockIdx.x * kHfBlock + threadIdx.x;
  if (j >= n_rows) return;
  const uint32_t id = index ? (uint32_t)index[j] : j;
  const float4 g = id < n_points ? reinterpret_cast<const float4*>(g_raw)[id] : make_float4(0.f, 0.f, 0.f, 0.f);
  float* __restrict__ c = g_rgb + (size_t)j * 3;
  c[0] = g.x; c[1] = g.y; c[2] = g.z;
  g_sigma_rows[j] = g.w;
}

bool hf_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the sizes every entry with rows checks: 1 <= n_rows <= n_points <= 2^31 - 1
int hf_check_rows(const char* entry, int64_t n_rows, int64_t n_points) {
  if (n_points <= 0 || n_points > 0x7fffffffLL)
    return fail(NERF_ERR_INVALID_ARG, "%s: the number of point ids (n_rays * n_samples) must be in [1, 2^31 - 1]", entry);
  if (n_rows <= 0 || n_rows > n_points) return fail(NERF_ERR_INVALID_ARG, "%s: n_rows must be in [1, number of point ids]", entry);
  return NERF_OK;
}

// ... and those with rays: n_samples in [1, 192], n_rays >= 1, n_rays * n_samples <= 2^31 - 1
int hf_check_rays(const char* entry, int64_t n_rays, int32_t n_samples, int64_t n_rows) {
  if (n_samples < 1 || n_samples > kHfMaxSamples) return fail(NERF_ERR_INVALID_ARG, "%s: n_samples must be in [1, 192]", entry);
  if (n_rays <= 0 || n_rays > 0x7fffffffLL / n_samples)
    return fail(NERF_ERR_INVALID_ARG, "%s: n_rays must be positive and n_rays * n_samples at most 2^31 - 1", entry);
  return hf_check_rows(entry, n_rows, n_rays * n_samples);
}

inline dim3 hf_grid(int64_t threads) { return dim3((unsigned)((threads + kHfBlock - 1) / kHfBlock)); }

// ---- the spatial adjoint (include/nerf_mi355x_field.h, DESIGN.md section 2.14.1) ------------------------------------------------------
// Lane mappings:
//   density_seed            one thread per float4 of a seed row (4 per row); thread 0 of a row reads the row's sigma
//   points_backward (rows)  one thread per row: the forward's p again, three divisions, three plain stores at slot j or at the id
//   points_backward (rays)  one wave per ray: the run by binary search, lane l takes rows a + l, a + l + 64, ...; xor butterfly
//   sh_gradient             the same walk over 16 columns of g_cin; lanes 0..3 store one float4 each
//   sh4_encode_backward     one thread per ray

// row j -> the point id clamped for READS, the forward's p and the sample's depth (0 in point mode)
__device__ __forceinline__ void hf_row_point(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                             const float* __restrict__ tvals, long long t_ray_stride, uint32_t n_samples, uint32_t id,
                                             float p[3], float& t) {
  const uint32_t ray = id / n_samples, s = id - ray * n_samples;
  const float* __restrict__ o = rays_o + (size_t)ray * 3;
  p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
  t = 0.0f;
  if (rays_d) {
    const float* __restrict__ d = rays_d + (size_t)ray * 3;
    t = tvals[(long long)ray * t_ray_stride + s];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = __fadd_rn(p[a], __fmul_rn(d[a], t));
  }
}

__device__ __forceinline__ float hf_clamp_adjoint(float p, float lo, float hi, float g, float extent) {
  return (p >= lo && p <= hi) ? __fdiv_rn(g, extent) : 0.0f;
}

// the first row in [0, n_rows) whose id is >= target (n_rows if none); index == NULL: the ids are the row numbers
__device__ __forceinline__ uint32_t hf_lower_bound(const int* __restrict__ index, uint32_t n_rows, long long target) {
  if (!index) return (uint32_t)(target < (long long)n_rows ? target : (long long)n_rows);
  uint32_t lo = 0, hi = n_rows;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((long long)index[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float hf_wave_sum(float v) {
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) v = __fadd_rn(v, __shfl_xor(v, h));
  return v;
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_density_seed_kernel(const float* __restrict__ sigma, long long sigma_stride, uint32_t n_rows, int positive_only,
                                    float* __restrict__ seed) {
  const unsigned long long t = (unsigned long long)blockIdx.x * kHfBlock + threadIdx.x;
  const uint32_t q = (uint32_t)(t & 3u);
  if ((t >> 2) >= n_rows) return;
  const uint32_t j = (uint32_t)(t >> 2);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q == 0) v.x = (positive_only && !(sigma[(long long)j * sigma_stride] > 0.0f)) ? 0.0f : 1.0f;
  reinterpret_cast<float4*>(seed + (size_t)j * kHfGeo)[q] = v;
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_points_backward_rows_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                            const float* __restrict__ tvals, long long t_ray_stride, uint32_t n_samples,
                                            const int* __restrict__ index, uint32_t n_rows, uint32_t n_points, HfBox box, float extent,
                                            const float* __restrict__ g_x, int by_id, float* __restrict__ g_p) {
  const uint32_t j = blockIdx.x * kHfBlock + threadIdx.x;
  if (j >= n_rows) return;
  const uint32_t id = index ? (uint32_t)index[j] : j;
  if (by_id && id >= n_points) return;                         // never a store address
  float p[3], t;
  hf_row_point(rays_o, rays_d, tvals, t_ray_stride, n_samples, id < n_points ? id : n_points - 1, p, t);
  const float* __restrict__ g = g_x + (size_t)j * 3;
  float* __restrict__ out = g_p + (size_t)(by_id ? id : j) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = hf_clamp_adjoint(p[a], box.lo[a], box.hi[a], g[a], extent);
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_points_backward_rays_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                            const float* __restrict__ tvals, long long t_ray_stride, uint32_t n_rays, uint32_t n_samples,
                                            const int* __restrict__ index, uint32_t n_rows, uint32_t n_points, HfBox box, float extent,
                                            const float* __restrict__ g_x, const float* __restrict__ g_dview,
                                            float* __restrict__ g_o, float* __restrict__ g_d) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long ray = (unsigned long long)blockIdx.x * (kHfBlock / 64) + (threadIdx.x >> 6);
  if (ray >= n_rays) return;                                   // (whole waves; no barrier below)
  const long long first = (long long)ray * n_samples;
  const uint32_t a0 = hf_lower_bound(index, n_rows, first), b0 = hf_lower_bound(index, n_rows, first + n_samples);
  float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
  for (unsigned long long j = (unsigned long long)a0 + lane; j < b0; j += 64) {
    uint32_t id = index ? (uint32_t)index[j] : (uint32_t)j;
    if (id >= n_points) id = n_points - 1;                     // a read only
    float p[3], t;
    hf_row_point(rays_o, rays_d, tvals, t_ray_stride, n_samples, id, p, t);
    const float* __restrict__ g = g_x + (size_t)j * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float gp = hf_clamp_adjoint(p[a], box.lo[a], box.hi[a], g[a], extent);
      so[a] = __fadd_rn(so[a], gp);
      sd[a] = __fadd_rn(sd[a], __fmul_rn(t, gp));
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { so[a] = hf_wave_sum(so[a]); sd[a] = hf_wave_sum(sd[a]); }
  if (lane < 3) {
    const float o_l = lane == 0 ? so[0] : lane == 1 ? so[1] : so[2];
    const float d_l = lane == 0 ? sd[0] : lane == 1 ? sd[1] : sd[2];
    if (g_o) g_o[ray * 3 + lane] = o_l;
    if (g_d) g_d[ray * 3 + lane] = g_dview ? __fadd_rn(d_l, g_dview[ray * 3 + lane]) : d_l;
  }
}

__global__ __launch_bounds__(kHfBlock)
void nerf_field_sh_gradient_kernel(const float* __restrict__ g_cin, const int* __restrict__ index, uint32_t n_rows, uint32_t n_rays,
                                   uint32_t n_samples, float* __restrict__ g_sh) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long ray = (unsigned long long)blockIdx.x * (kHfBlock / 64) + (threadIdx.x >> 6);
  if (ray >= n_rays) return;                                   // (whole waves; no barrier below)
  const long long first = (long long)ray * n_samples;
  const uint32_t a0 = hf_lower_bound(index, n_rows, first), b0 = hf_lower_bound(index, n_rows, first + n_samples);
  float4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (unsigned long long j = (unsigned long long)a0 + lane; j < b0; j += 64) {
    const float4* __restrict__ row = reinterpret_cast<const float4*>(g_cin + (size_t)j * (2 * kHfGeo) + kHfGeo);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = row[q];
      acc[q].x = __fadd_rn(acc[q].x, v.x); acc[q].y = __fadd_rn(acc[q].y, v.y);
      acc[q].z = __fadd_rn(acc[q].z, v.z); acc[q].w = __fadd_rn(acc[q].w, v.w);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q].x = hf_wave_sum(acc[q].x); acc[q].y = hf_wave_sum(acc[q].y);
    acc[q].z = hf_wave_sum(acc[q].z); acc[q].w = hf_wave_sum(acc[q].w);
  }
  float4* __restrict__ out = reinterpret_cast<float4*>(g_sh + (size_t)ray * kHfGeo);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (lane == (uint32_t)q) out[q] = acc[q];
}

__global__ __launch_bounds__(kHfBlock)
void nerf_sh4_encode_backward_kernel(const float* __restrict__ rays_d, const float* __restrict__ g_sh, uint32_t n_rays,
                                     float* __restrict__ g_dview) {
  const uint32_t r = blockIdx.x * kHfBlock + threadIdx.x;
  if (r >= n_rays) return;
  const float* __restrict__ d = rays_d + (size_t)r * 3;
  float x = d[0], y = d[1], z = d[2];
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
  const float nrm = sqrtf(s);                                  // correctly rounded, as in nerf_sh4_encode_kernel
  x = __fdiv_rn(x, nrm); y = __fdiv_rn(y, nrm); z = __fdiv_rn(z, nrm);
  float g[16];
  const float4* __restrict__ gin = reinterpret_cast<const float4*>(g_sh + (size_t)r * kHfGeo);
#pragma unroll
  for (int q = 0; q < 4; ++q) { const float4 v = gin[q]; g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w; }
  constexpr float c1 = 0.48860251190291987f, c2 = 1.0925484305920792f, c3 = 0.94617469575755997f, c4 = 0.54627421529603959f,
                  c5 = 0.59004358992664352f, c6 = 2.8906114426405538f, c7 = 0.45704579946446572f, c8 = 0.3731763325901154f,
                  c9 = 1.4453057213202769f;
  const float q5 = __fsub_rn(1.0f, __fmul_rn(__fmul_rn(5.0f, z), z));                     // 1 - 5*z*z
  const float m = __fsub_rn(__fmul_rn(y, y), __fmul_rn(x, x));                            // y*y - x*x
  const float c5m3 = __fmul_rn(__fmul_rn(c5, m), 3.0f);
  const float c5xy = __fmul_rn(__fmul_rn(c5, x), y);
  const float c7q = __fmul_rn(c7, q5);
  float gx = __fmul_rn(g[3], -c1);
  gx = __fadd_rn(gx, __fmul_rn(g[4], __fmul_rn(c2, y)));
  gx = __fadd_rn(gx, __fmul_rn(g[7], __fmul_rn(-c2, z)));
  gx = __fadd_rn(gx, __fmul_rn(g[8], __fmul_rn(__fmul_rn(c4, x), 2.0f)));
  gx = __fadd_rn(gx, __fmul_rn(g[9], __fmul_rn(c5xy, -6.0f)));
  gx = __fadd_rn(gx, __fmul_rn(g[10], __fmul_rn(__fmul_rn(c6, y), z)));
  gx = __fadd_rn(gx, __fmul_rn(g[13], c7q));
  gx = __fadd_rn(gx, __fmul_rn(g[14], __fmul_rn(__fmul_rn(__fmul_rn(c9, x), z), 2.0f)));
  gx = __fadd_rn(gx, __fmul_rn(g[15], c5m3));
  float gy = __fmul_rn(g[1], -c1);
  gy = __fadd_rn(gy, __fmul_rn(g[4], __fmul_rn(c2, x)));
  gy = __fadd_rn(gy, __fmul_rn(g[5], __fmul_rn(-c2, z)));
  gy = __fadd_rn(gy, __fmul_rn(g[8], __fmul_rn(__fmul_rn(c4, y), -2.0f)));
  gy = __fadd_rn(gy, __fmul_rn(g[9], c5m3));
  gy = __fadd_rn(gy, __fmul_rn(g[10], __fmul_rn(__fmul_rn(c6, x), z)));
  gy = __fadd_rn(gy, __fmul_rn(g[11], c7q));
  gy = __fadd_rn(gy, __fmul_rn(g[14], __fmul_rn(__fmul_rn(__fmul_rn(c9, y), z), -2.0f)));
  gy = __fadd_rn(gy, __fmul_rn(g[15], __fmul_rn(c5xy, 6.0f)));
  float gz = __fmul_rn(g[2], c1);
  gz = __fadd_rn(gz, __fmul_rn(g[5], __fmul_rn(-c2, y)));
  gz = __fadd_rn(gz, __fmul_rn(g[6], __fmul_rn(__fmul_rn(c3, z), 2.0f)));
  gz = __fadd_rn(gz, __fmul_rn(g[7], __fmul_rn(-c2, x)));
  gz = __fadd_rn(gz, __fmul_rn(g[10], __fmul_rn(__fmul_rn(c6, x), y)));
  gz = __fadd_rn(gz, __fmul_rn(g[11], __fmul_rn(__fmul_rn(__fmul_rn(c7, y), z), -10.0f)));
  gz = __fadd_rn(gz, __fmul_rn(g[12], __fmul_rn(c8, __fsub_rn(__fmul_rn(__fmul_rn(15.0f, z), z), 3.0f))));
  gz = __fadd_rn(gz, __fmul_rn(g[13], __fmul_rn(__fmul_rn(__fmul_rn(c7, x), z), -10.0f)));
  gz = __fadd_rn(gz, __fmul_rn(g[14], __fmul_rn(c9, __fsub_rn(__fmul_rn(x, x), __fmul_rn(y, y)))));
  const float w = __fadd_rn(__fadd_rn(__fmul_rn(x, gx), __fmul_rn(y, gy)), __fmul_rn(z, gz));
  float* __restrict__ out = g_dview + (size_t)r * 3;
  out[0] = __fdiv_rn(__fsub_rn(gx, __fmul_rn(x, w)), nrm);
  out[1] = __fdiv_rn(__fsub_rn(gy, __fmul_rn(y, w)), nrm);
  out[2] = __fdiv_rn(__fsub_rn(gz, __fmul_rn(z, w)), nrm);
}

}  // namespace

extern "C" {

int32_t nerf_sh4_encode(const float* rays_d, int64_t n_rays, float* sh, void* stream) {
  if (n_rays <= 0 || n_rays > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sh4_encode: n_rays must be in [1, 2^31 - 1]");
  if (!rays_d || !sh) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sh4_encode: null argument");
  if (!hf_aligned16(sh)) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_sh4_encode: sh must be aligned to 16 bytes");
  return NERF_LAUNCH(nerf_sh4_encode_kernel, hf_grid(n_rays), dim3(kHfBlock), (hipStream_t)stream, rays_d, (uint32_t)n_rays, sh);
}

int32_t nerf_field_points(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                          int32_t n_samples, const int32_t* index, int64_t n_rows, const float box_min[3], const float box_max[3],
                          float extent, float* x, void* stream) {
  const char* entry = "nerf_field_points";
  const int rc = hf_check_rays(entry, n_rays, n_samples, n_rows);
  if (rc) return rc;
  if (!rays_o || !box_min || !box_max || !x) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (rays_d ? (!tvals || t_ray_stride < 0) : n_samples != 1)
    return fail(NERF_ERR_INVALID_ARG, "%s: rays need rays_d, tvals and a stride >= 0; point mode (rays_d == NULL) needs n_samples == 1", entry);
  if (!(extent > 0.0f)) return fail(NERF_ERR_INVALID_ARG, "%s: extent must be positive", entry);
  HfBox box;
  for (int a = 0; a < 3; ++a) { box.lo[a] = box_min[a]; box.hi[a] = box_max[a]; }
  return NERF_LAUNCH(nerf_field_points_kernel, hf_grid(n_rows), dim3(kHfBlock), (hipStream_t)stream, rays_o, rays_d, tvals,
                     (long long)t_ray_stride, (uint32_t)n_samples, index, (uint32_t)n_rows, (uint32_t)(n_rays * n_samples), box, extent, x);
}

int32_t nerf_field_color_inputs(const float* geo, const float* sh, const int32_t* index, int64_t n_rows, int64_t n_rays,
                                int32_t n_samples, float* cin, float* sigma_rows, void* stream) {
  const char* entry = "nerf_field_color_inputs";
  const int rc = hf_check_rays(entry, n_rays, n_samples, n_rows);
  if (rc) return rc;
  if (!geo || !sh || !cin || !sigma_rows) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hf_aligned16(geo) || !hf_aligned16(sh) || !hf_aligned16(cin))
    return fail(NERF_ERR_INVALID_ARG, "%s: geo, sh and cin must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_field_color_inputs_kernel, hf_grid(n_rows * 8), dim3(kHfBlock), (hipStream_t)stream, geo, sh, index,
                     (uint32_t)n_rows, (uint32_t)n_samples, (uint32_t)(n_rays * n_samples), cin, sigma_rows);
}

int32_t nerf_field_color_inputs_backward(const float* g_cin, const float* g_sigma_rows, int64_t n_rows, float* g_geo, void* stream) {
  const char* entry = "nerf_field_color_inputs_backward";
  const int rc = hf_check_rows(entry, n_rows, 0x7fffffffLL);
  if (rc) return rc;
  if (!g_cin || !g_sigma_rows || !g_geo) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hf_aligned16(g_cin) || !hf_aligned16(g_geo)) return fail(NERF_ERR_INVALID_ARG, "%s: g_cin and g_geo must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_field_color_inputs_backward_kernel, hf_grid(n_rows * 4), dim3(kHfBlock), (hipStream_t)stream, g_cin,
                     g_sigma_rows, (uint32_t)n_rows, g_geo);
}

int32_t nerf_field_raw_scatter(const float* rgb, const float* sigma_rows, const int32_t* index, int64_t n_rows, int64_t n_points,
                               float* raw, void* stream) {
  const char* entry = "nerf_field_raw_scatter";
  const int rc = hf_check_rows(entry, n_rows, n_points);
  if (rc) return rc;
  if (!rgb || !sigma_rows || !raw) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hf_aligned16(raw)) return fail(NERF_ERR_INVALID_ARG, "%s: raw must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_field_raw_scatter_kernel, hf_grid(n_rows), dim3(kHfBlock), (hipStream_t)stream, rgb, sigma_rows, index,
                     (uint32_t)n_rows, (uint32_t)n_points, raw);
}

int32_t nerf_field_raw_gather(const float* g_raw, const int32_t* index, int64_t n_rows, int64_t n_points, float* g_rgb,
                              float* g_sigma_rows, void* stream) {
  const char* entry = "nerf_field_raw_gather";
  const int rc = hf_check_rows(entry, n_rows, n_points);
  if (rc) return rc;
  if (!g_raw || !g_rgb || !g_sigma_rows) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hf_aligned16(g_raw)) return fail(NERF_ERR_INVALID_ARG, "%s: g_raw must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_field_raw_gather_kernel, hf_grid(n_rows), dim3(kHfBlock), (hipStream_t)stream, g_raw, index,
                     (uint32_t)n_rows, (uint32_t)n_points, g_rgb, g_sigma_rows);
}

// ---- include/nerf_mi355x_field.h ---------------------------------------------------------------------------------------------------------
int32_t nerf_field_density_seed(const float* sigma, int64_t sigma_stride, int64_t n_rows, int32_t positive_only, float* seed,
                                void* stream) {
  const char* entry = "nerf_field_density_seed";
  const int rc = hf_check_rows(entry, n_rows, 0x7fffffffLL);
  if (rc) return rc;
  if (!sigma || !seed) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (sigma_stride < 1) return fail(NERF_ERR_INVALID_ARG, "%s: sigma_stride must be at least 1", entry);
  if (!hf_aligned16(seed)) return fail(NERF_ERR_INVALID_ARG, "%s: seed must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_field_density_seed_kernel, hf_grid(n_rows * 4), dim3(kHfBlock), (hipStream_t)stream, sigma,
                     (long long)sigma_stride, (uint32_t)n_rows, (int)(positive_only != 0), seed);
}

int32_t nerf_field_points_backward(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                                   int32_t n_samples, const int32_t* index, int64_t n_rows, const float box_min[3],
                                   const float box_max[3], float extent, const float* g_x, const float* g_rays_d_view, int32_t by_id,
                                   float* g_p, float* g_rays_o, float* g_rays_d, void* stream) {
  const char* entry = "nerf_field_points_backward";
  int rc = hf_check_rays(entry, n_rays, n_samples, n_rows);
  if (rc) return rc;
  if (!rays_o || !box_min || !box_max || !g_x) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (rays_d ? (!tvals || t_ray_stride < 0) : (n_samples != 1 || g_rays_o || g_rays_d || g_rays_d_view))
    return fail(NERF_ERR_INVALID_ARG, "%s: rays need rays_d, tvals and a stride >= 0; point mode (rays_d == NULL) needs n_samples == 1 "
                "and has no per-ray output", entry);
  if (!(extent > 0.0f)) return fail(NERF_ERR_INVALID_ARG, "%s: extent must be positive", entry);
  if (!g_p && !g_rays_o && !g_rays_d) return fail(NERF_ERR_INVALID_ARG, "%s: no output is given", entry);
  if (g_rays_d_view && !g_rays_d) return fail(NERF_ERR_INVALID_ARG, "%s: g_rays_d_view needs g_rays_d", entry);
  HfBox box;
  for (int a = 0; a < 3; ++a) { box.lo[a] = box_min[a]; box.hi[a] = box_max[a]; }
  const uint32_t n_points = (uint32_t)(n_rays * n_samples);
  if (g_p) {
    rc = NERF_LAUNCH(nerf_field_points_backward_rows_kernel, hf_grid(n_rows), dim3(kHfBlock), (hipStream_t)stream, rays_o, rays_d, tvals,
                     (long long)t_ray_stride, (uint32_t)n_samples, index, (uint32_t)n_rows, n_points, box, extent, g_x,
                     (int)(by_id != 0), g_p);
    if (rc) return rc;
  }
  if (!g_rays_o && !g_rays_d) return NERF_OK;
  return NERF_LAUNCH(nerf_field_points_backward_rays_kernel, hf_grid(n_rays * 64), dim3(kHfBlock), (hipStream_t)stream, rays_o, rays_d,
                     tvals, (long long)t_ray_stride, (uint32_t)n_rays, (uint32_t)n_samples, index, (uint32_t)n_rows, n_points, box,
                     extent, g_x, g_rays_d_view, g_rays_o, g_rays_d);
}

int32_t nerf_field_sh_gradient(const float* g_cin, const int32_t* index, int64_t n_rows, int64_t n_rays, int32_t n_samples,
                               float* g_sh, void* stream) {
  const char* entry = "nerf_field_sh_gradient";
  const int rc = hf_check_rays(entry, n_rays, n_samples, n_rows);
  if (rc) return rc;
  if (!g_cin || !g_sh) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hf_aligned16(g_cin) || !hf_aligned16(g_sh)) return fail(NERF_ERR_INVALID_ARG, "%s: g_cin and g_sh must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_field_sh_gradient_kernel, hf_grid(n_rays * 64), dim3(kHfBlock), (hipStream_t)stream, g_cin, index,
                     (uint32_t)n_rows, (uint32_t)n_rays, (uint32_t)n_samples, g_sh);
}

int32_t nerf_sh4_encode_backward(const float* rays_d, const float* g_sh, int64_t n_rays, float* g_rays_d_view, void* stream) {
  const char* entry = "nerf_sh4_encode_backward";
  if (n_rays <= 0 || n_rays > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s: n_rays must be in [1, 2^31 - 1]", entry);
  if (!rays_d || !g_sh || !g_rays_d_view) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hf_aligned16(g_sh)) return fail(NERF_ERR_INVALID_ARG, "%s: g_sh must be aligned to 16 bytes", entry);
  return NERF_LAUNCH(nerf_sh4_encode_backward_kernel, hf_grid(n_rays), dim3(kHfBlock), (hipStream_t)stream, rays_d, g_sh,
                     (uint32_t)n_rays, g_rays_d_view);
}

}  // extern "C"
