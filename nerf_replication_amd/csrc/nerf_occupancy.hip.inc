// Occupancy grid: a bitfield over the cells of a density grid, and the per-sample lookup that culls empty space from a render
// (DESIGN.md section 2.9; the definitions are in include/nerf_mi355x.h, nerf_occupancy_*).
// Needs, ahead of it, nerf_mlp_launch.hip.inc (masked_sizes_ok) and nerf_frame.hip.inc (render_frame, RenderOccupancy,
// render_workspace_bytes; the tally of the points a pass evaluated lives there too, with its caller).
#include "nerf_host.h"
//
// Both kernels are memory-trivial: the bitfield is (nx-1)(ny-1)(nz-1) / 8 bytes (2 MB at 256^3) and stays in L2; the build reads
// the field (2r + 2)^3 times per cell out of the same cache, once per grid; the mark reads 4 bytes and writes 1 per sample.

namespace {

constexpr int kOccBlock = 256;

struct OccGrid {
  int cx, cy, cz;          // cells per axis = points - 1
  long long cells;
};

// One wave per 64-bit word (two 32-bit words of the bitfield): lane l decides cell 64 w + l, the ballot is the word.  Cells past
// the last one vote 0: the tail bits and the pad word of an odd word count are written as zeros.  No atomics.
__global__ __launch_bounds__(kOccBlock)
void nerf_occupancy_build_kernel(const float* __restrict__ field, long long stride, OccGrid G, float level, int dilate,
                                 long long n_words64, unsigned* __restrict__ bits) {
  const long long w = (long long)blockIdx.x * (kOccBlock / 64) + (threadIdx.x >> 6);       // wave-uniform
  if (w >= n_words64) return;
  const int lane = threadIdx.x & 63;
  const long long id = w * 64 + lane;
  bool occ = false;
  if (id < G.cells) {
    const int k = (int)(id % G.cz);
    const long long r = id / G.cz;
    const int j = (int)(r % G.cy), i = (int)(r / G.cy);
    const int ny = G.cy + 1, nz = G.cz + 1;
    const int i0 = max(i - dilate, 0), i1 = min(i + 1 + dilate, G.cx);                      // point indices, clipped to the grid
    const int j0 = max(j - dilate, 0), j1 = min(j + 1 + dilate, G.cy);
    const int k0 = max(k - dilate, 0), k1 = min(k + 1 + dilate, G.cz);
    for (int a = i0; a <= i1 && !occ; ++a)
      for (int b = j0; b <= j1 && !occ; ++b) {
        const float* line = field + ((long long)a * ny + b) * nz * stride;
        for (int c = k0; c <= k1; ++c) {
          const float f = line[c * stride];
          occ = occ || !(f <= level);                  // f > level, or NaN
        }
      }
  }
  const unsigned long long m = __builtin_amdgcn_ballot_w64(occ);
  if (lane == 0) {
    bits[2 * w] = (unsigned)(m & 0xffffffffull);
    bits[2 * w + 1] = (unsigned)(m >> 32);
  }
}

// The grid's memory across refreshes: one thread per grid point.  age counts the refreshes since the point was last above the level
// (0: now; saturates at 255), `on` is > 0 while that is fewer than `hold` refreshes ago.  `on` may be `field` itself (stride 1): each
// thread reads its own point before it writes it, so neither pointer is __restrict__.
__global__ __launch_bounds__(kOccBlock)
void nerf_occupancy_age_kernel(const float* field, long long stride, long long n_points, float level, int hold,
                               unsigned char* __restrict__ age, float* on) {
  const long long p = (long long)blockIdx.x * kOccBlock + threadIdx.x;
  if (p >= n_points) return;
  const float f = field[p * stride];
  const bool hit = !(f <= level);                          // f > level, or NaN
  const int a = hit ? 0 : min((int)age[p] + 1, 255);
  age[p] = (unsigned char)a;
  on[p] = a < hold ? 1.0f : -1.0f;
}

struct OccLookup {
  int cx, cy, cz;
  float min[3], inv[3];
};

// One thread per (ray, sample): consecutive threads read consecutive depths and store consecutive bytes.
__global__ __launch_bounds__(kOccBlock)
void nerf_occupancy_mark_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ tvals,
                                long long t_ray_stride, long long n_points, int n_samples, const unsigned* __restrict__ bits,
                                OccLookup L, int and_with_existing, unsigned char* __restrict__ valid) {
  const long long e = (long long)blockIdx.x * kOccBlock + threadIdx.x;
  if (e >= n_points) return;
  const long long ray = e / n_samples;
  const int s = (int)(e - ray * n_samples);
  const float t = tvals[ray * t_ray_stride + s];
  float c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = __fadd_rn(rays_o[ray * 3 + a], __fmul_rn(rays_d[ray * 3 + a], t));       // the forward kernels' two roundings
    c[a] = floorf(__fmul_rn(__fsub_rn(x, L.min[a]), L.inv[a]));
  }
  // outside the box (or NaN: every comparison false) counts as occupied
  const bool in_box = c[0] >= 0.0f && c[0] <= (float)(L.cx - 1) && c[1] >= 0.0f && c[1] <= (float)(L.cy - 1) &&
                      c[2] >= 0.0f && c[2] <= (float)(L.cz - 1);
  bool keep = true;
  if (in_box) {
    const unsigned id = ((unsigned)c[0] * (unsigned)L.cy + (unsigned)c[1]) * (unsigned)L.cz + (unsigned)c[2];     // < 2^31
    keep = (bits[id >> 5] >> (id & 31u)) & 1u;
  }
  valid[e] = (unsigned char)((and_with_existing ? valid[e] != 0 : true) && keep);
}

// 0: sizes fine; the grid as OccGrid.  Every dimension >= 2, at most 2^31 - 1 points (cell ids are int32)
int occ_sizes(const char* entry, const int32_t dims[3], OccGrid& G) {
  if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return fail(NERF_ERR_INVALID_ARG, "%s: every grid dimension must be >= 2", entry);
  const long long n = (long long)dims[0] * dims[1];
  if (n > 0x7fffffffLL / dims[2]) return fail(NERF_ERR_INVALID_ARG, "%s: more than 2^31 - 1 grid points", entry);
  G.cx = dims[0] - 1; G.cy = dims[1] - 1; G.cz = dims[2] - 1;
  G.cells = (long long)G.cx * G.cy * G.cz;
  return NERF_OK;
}

int occ_lookup(const char* entry, const int32_t dims[3], const float box_min[3], const float inv_step[3], OccLookup& L) {
  if (!dims || !box_min || !inv_step) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  OccGrid G;
  const int rc = occ_sizes(entry, dims, G);
  if (rc) return rc;
  L.cx = G.cx; L.cy = G.cy; L.cz = G.cz;
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(box_min[a]) || !isfinite(inv_step[a]) || !(inv_step[a] > 0.0f))
      return fail(NERF_ERR_INVALID_ARG, "%s: box_min must be finite and inv_step finite and positive", entry);
    L.min[a] = box_min[a]; L.inv[a] = inv_step[a];
  }
  return NERF_OK;
}

}  // namespace

extern "C" {

int64_t nerf_occupancy_words(int32_t nx, int32_t ny, int32_t nz) {
  const int32_t dims[3] = {nx, ny, nz};
  OccGrid G;
  if (occ_sizes("nerf_occupancy_words", dims, G)) return -1;
  return 2 * ((G.cells + 63) / 64);
}

int32_t nerf_occupancy_build(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level, int32_t dilate,
                             uint32_t* bits, void* stream) {
  const int32_t dims[3] = {nx, ny, nz};
  OccGrid G;
  const int rc = occ_sizes("nerf_occupancy_build", dims, G);
  if (rc) return rc;
  if (stride < 1 || dilate < 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_build: stride must be >= 1 and dilate >= 0");
  if (!field || !bits) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_build: null argument");
  const int reach = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);       // a larger dilation reads the whole grid just the same
  const long long n_words64 = (G.cells + 63) / 64;
  const long long blocks = (n_words64 + kOccBlock / 64 - 1) / (kOccBlock / 64);
  return NERF_LAUNCH(nerf_occupancy_build_kernel, dim3((unsigned)blocks), dim3(kOccBlock), (hipStream_t)stream, field,
                     (long long)stride, G, level, dilate < reach ? dilate : reach, n_words64, bits);
}

int32_t nerf_occupancy_age(const float* field, int64_t stride, int64_t n_points, float level, int32_t hold, uint8_t* age, float* on,
                           void* stream) {
  if (n_points < 0 || n_points > (int64_t)0x7fffffff) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_age: n_points must be in [0, 2^31 - 1]");
  if (stride < 1 || hold < 1 || hold > 255) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_age: stride must be >= 1 and hold in [1, 255]");
  if (n_points == 0) return NERF_OK;
  if (!field || !age || !on) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_age: null argument");
  return NERF_LAUNCH(nerf_occupancy_age_kernel, dim3((unsigned)((n_points + kOccBlock - 1) / kOccBlock)), dim3(kOccBlock),
                     (hipStream_t)stream, field, (long long)stride, (long long)n_points, level, hold, age, on);
}

int32_t nerf_occupancy_mark(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                            int32_t n_samples, const uint32_t* bits, const int32_t dims[3], const float box_min[3],
                            const float inv_step[3], int32_t and_with_existing, uint8_t* valid, void* stream) {
  if (!masked_sizes_ok(n_rays, n_samples, t_ray_stride)) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_mark: bad size");
  OccLookup L;
  const int rc = occ_lookup("nerf_occupancy_mark", dims, box_min, inv_step, L);
  if (rc) return rc;
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !tvals || !bits || !valid) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_occupancy_mark: null argument");
  const long long np = n_rays * (long long)n_samples;
  return NERF_LAUNCH(nerf_occupancy_mark_kernel, dim3((unsigned)((np + kOccBlock - 1) / kOccBlock)), dim3(kOccBlock),
                     (hipStream_t)stream, rays_o, rays_d, tvals, (long long)t_ray_stride, np, n_samples, bits, L, and_with_existing,
                     valid);
}

int64_t nerf_render_occupancy_workspace_bytes(int64_t n_rays_frame, int32_t n_importance, int32_t fast_sampling) {
  return render_workspace_bytes(n_rays_frame, n_importance, fast_sampling, false, true);
}

int32_t nerf_render_forward_occupancy(const float* rays_o, const float* rays_d, int64_t n_rays,
                                      const void* packed_coarse, const void* packed_fine,
                                      const float* t_coarse, const float* u, int32_t n_importance,
                                      int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                                      float weights_threshold, const uint32_t* occ_coarse, const uint32_t* occ_fine,
                                      const int32_t dims[3], const float box_min[3], const float inv_step[3],
                                      int64_t* evaluated, void* workspace, int64_t workspace_bytes,
                                      float* rgb, float* depth, void* stream) {
  const char* entry = "nerf_render_forward_occupancy";
  // the fp16 far-plane guard re-evaluates the last sample of every ray: not defined on a culled list
  if (precision != NERF_PREC_F32 && precision != NERF_PREC_F32X) return fail(NERF_ERR_UNSUPPORTED, "%s: f32 or f32x only", entry);
  if (n_rays > (int64_t)0x7fffffff / (NERF_N_SAMPLES + NERF_N_IMPORTANCE))
    return fail(NERF_ERR_INVALID_ARG, "%s: at most 11 184 810 rays per call (n_rays * 192 point ids must fit in int32): split the frame", entry);
  RenderOccupancy occ{};
  occ.coarse = occ_coarse; occ.fine = n_importance ? occ_fine : nullptr; occ.evaluated = (long long*)evaluated;
  if (occ.coarse || occ.fine) {
    OccLookup L;
    const int rc = occ_lookup(entry, dims, box_min, inv_step, L);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) { occ.dims[a] = dims[a]; occ.box_min[a] = box_min[a]; occ.inv_step[a] = inv_step[a]; }
  }
  if (evaluated && hipMemsetAsync(evaluated, 0, 2 * sizeof(int64_t), (hipStream_t)stream) != hipSuccess)
    return fail(NERF_ERR_HIP, "%s: memset failed", entry);
  return render_frame(entry, rays_o, rays_d, n_rays, packed_coarse, packed_fine, t_coarse, u, nullptr, nullptr, false, n_importance,
                      white_bkgd, precision, fast_sampling, weights_threshold, workspace, workspace_bytes, rgb, depth, stream, &occ);
}

}  // extern "C"
