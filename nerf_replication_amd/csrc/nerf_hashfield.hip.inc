// Ray-side glue of the hash-grid radiance field (DESIGN.md section 2.14): what sits between nerf_occupancy_mark / nerf_compact_valid,
// nerf_hashgrid_forward, nerf_fused_mlp_forward and nerf_composite.  Included at the end of nerf_kernels.hip (uses its fail /
// NERF_LAUNCH); the declarations and every formula are in include/nerf_mi355x_nn.h.  fp32 throughout; the unit is compiled with
// -ffp-contract=off and every operation below is written with its own rounding, so each kernel is bit for bit the fp32 restatement in
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

}  // extern "C"
