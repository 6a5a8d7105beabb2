// The rank-factorised deformation field of a dynamic scene (DESIGN.md section 2.15): the warp of the normalised sample positions, its
// table gradient, and the repacking of the tables.  The declarations, the device layout and every formula are in
// include/nerf_mi355x_deform.h.  fp32 throughout; the unit is compiled with -ffp-contract=off and every operation below is written with
// its own rounding, so the forward is bit for bit the restatement in tests/deform_reference.py.
//
// Lane mappings:
//   forward / backward   one wave per row, lane = channel f: the 36 taps of a row (9 planes x 4) are 36 rows of 256 contiguous bytes of
//                        `packed`, each one request of the wave; the three sums over f are xor butterflies in the header's order.
//                        The backward recomputes the forward, then adds each tap's gradient back as ONE 256-byte wave-instruction of
//                        no-return global fp32 atomic adds (the contiguous form of the atomics' full rate).  Everything a row
//                        decides on (its id, time, gates) is the same in all 64 lanes: no divergence inside a wave.
//   pack / unpack        one workgroup per (table, plane, frame, 64 positions): a 64 x 64 tile goes through LDS, read with lanes along
//                        the source's inner axis and written with lanes along the destination's, both sides 256-byte rows.
#include "../../include/nerf_mi355x_deform.h"
#include "nerf_host.h"

namespace {

constexpr int kDfBlock = 256;            // 4 waves, one row each
constexpr int kDfF = 64;                 // channels: one wave's width
constexpr int kDfMaxSamples = 192;

struct DfArgs {
  const float* x;            // [n_rows,3]
  const float* time;         // [n_rays]
  const int* index;          // [n_rows] or NULL
  uint32_t n_rows, n_points, n_samples;
  const float* packed;       // [9][T][R][64]
  int T, R;
};

// What a row is, the same in every lane of its wave
struct DfRow {
  bool live;                 // its id is a point id
  bool nan_time, canonical;
  float x[3];
  float wx[3], ux[3], wy, uy;
  uint32_t tap[3];           // (y0 * R + x0_j) * 64: the offset of a00 inside a plane
};

__device__ __forceinline__ DfRow df_row(const DfArgs& a, uint32_t j) {
  DfRow r;
  const uint32_t id = a.index ? (uint32_t)a.index[j] : j;
  r.live = id < a.n_points;
  if (!r.live) return r;
  const float t = a.time[id / a.n_samples];
  r.nan_time = t != t;
  r.canonical = t == 0.0f;
  const float tc = fminf(fmaxf(t, 0.0f), (float)(a.T - 1));            // (a NaN t is handled by the caller: tc is then 0)
  const int y0 = min((int)floorf(tc), a.T - 2);
  r.wy = __fsub_rn(tc, (float)y0);
  r.uy = __fsub_rn(1.0f, r.wy);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.x[k] = a.x[(size_t)j * 3 + k];
    const float ix = __fmul_rn(r.x[k], (float)(a.R - 1));
    const int x0 = max(0, min((int)floorf(ix), a.R - 2));
    r.wx[k] = __fsub_rn(ix, (float)x0);
    r.ux[k] = __fsub_rn(1.0f, r.wx[k]);
    r.tap[k] = ((uint32_t)y0 * (uint32_t)a.R + (uint32_t)x0) * kDfF;
  }
  return r;
}

// v[i][j] of this lane's channel: all 36 loads are issued before the first is used
__device__ __forceinline__ void df_gather(const DfArgs& a, const DfRow& r, int lane, float v[3][3]) {
  const size_t plane = (size_t)a.T * a.R * kDfF, up = (size_t)a.R * kDfF;
  float tap[3][3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float* __restrict__ p = a.packed + (size_t)(i * 3 + j) * plane + r.tap[j] + lane;
      tap[i][j][0] = p[0];
      tap[i][j][1] = p[kDfF];
      tap[i][j][2] = p[up];
      tap[i][j][3] = p[up + kDfF];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float top = __fadd_rn(__fmul_rn(tap[i][j][0], r.ux[j]), __fmul_rn(tap[i][j][1], r.wx[j]));
      const float bot = __fadd_rn(__fmul_rn(tap[i][j][2], r.ux[j]), __fmul_rn(tap[i][j][3], r.wx[j]));
      v[i][j] = __fadd_rn(__fmul_rn(top, r.uy), __fmul_rn(bot, r.wy));
    }
}

// The sum over the 64 channels in the header's order; every lane ends with the same bits (fadd commutes)
__device__ __forceinline__ float df_sum64(float p) {
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) p = __fadd_rn(p, __shfl_xor(p, h, 64));
  return p;
}

__device__ __forceinline__ void df_delta(const float v[3][3], float delta[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) delta[i] = df_sum64(__fmul_rn(__fmul_rn(v[i][0], v[i][1]), v[i][2]));
}

__global__ __launch_bounds__(kDfBlock)
void nerf_deform_forward_kernel(DfArgs a, float* __restrict__ x_warped, float* __restrict__ delta_out) {
  const int lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * (kDfBlock / 64) + (threadIdx.x >> 6);
  if (j >= a.n_rows) return;
  const DfRow r = df_row(a, j);
  if (!r.live) return;
  float delta[3];
  if (r.nan_time) {
    delta[0] = delta[1] = delta[2] = __builtin_nanf("");
  } else if (r.canonical && !delta_out) {
    delta[0] = delta[1] = delta[2] = 0.0f;                       // not used: x' = x below
  } else {
    float v[3][3];
    df_gather(a, r, lane, v);
    df_delta(v, delta);
  }
  if (lane < 3) {                                                // lane k stores column k
    const float dk = lane == 0 ? delta[0] : lane == 1 ? delta[1] : delta[2];
    const float xk = lane == 0 ? r.x[0] : lane == 1 ? r.x[1] : r.x[2];
    if (delta_out) delta_out[(size_t)j * 3 + lane] = dk;
    if (x_warped) {
      float w = xk;
      if (r.nan_time) w = dk;
      else if (!r.canonical) w = fminf(fmaxf(__fadd_rn(xk, dk), 0.0f), 1.0f);
      x_warped[(size_t)j * 3 + lane] = w;
    }
  }
}

__global__ __launch_bounds__(kDfBlock)
void nerf_deform_backward_kernel(DfArgs a, const float* __restrict__ g_x_warped, const float* __restrict__ g_delta,
                                 float* __restrict__ g_packed) {
  const int lane = threadIdx.x & 63;
  const uint32_t j = blockIdx.x * (kDfBlock / 64) + (threadIdx.x >> 6);
  if (j >= a.n_rows) return;
  const DfRow r = df_row(a, j);
  if (!r.live || r.nan_time) return;
  const bool warped = g_x_warped && !r.canonical;
  if (!warped && !g_delta) return;
  float v[3][3], delta[3], g[3];
  df_gather(a, r, lane, v);
  df_delta(v, delta);
  bool any = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float s = __fadd_rn(r.x[i], delta[i]);
    g[i] = (warped && s >= 0.0f && s <= 1.0f) ? g_x_warped[(size_t)j * 3 + i] : 0.0f;
    if (g_delta) g[i] = __fadd_rn(g[i], g_delta[(size_t)j * 3 + i]);
    any = any || g[i] != 0.0f;
  }
  if (!any) return;
  const size_t plane = (size_t)a.T * a.R * kDfF, up = (size_t)a.R * kDfF;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (g[i] == 0.0f) continue;                                  // (the same in every lane)
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      const int pa = jj == 0 ? 1 : 0, pb = jj == 2 ? 1 : 2;      // the other two axes, ascending
      const float q = __fmul_rn(g[i], __fmul_rn(v[i][pa], v[i][pb]));
      const float qt = __fmul_rn(q, r.uy), qb = __fmul_rn(q, r.wy);
      float* __restrict__ p = g_packed + (size_t)(i * 3 + jj) * plane + r.tap[jj] + lane;
      atomicAdd(p, __fmul_rn(qt, r.ux[jj]));                     // results unused: the no-return form
      atomicAdd(p + kDfF, __fmul_rn(qt, r.wx[jj]));
      atomicAdd(p + up, __fmul_rn(qb, r.ux[jj]));
      atomicAdd(p + up + kDfF, __fmul_rn(qb, r.wx[jj]));
    }
  }
}

struct DfTables {                        // passed by value in the kernel arguments
  float* t[3];
};

// kToPacked: tables -> packed; else packed -> tables.  Block b = ((i * 3 + j) * T + y) * tiles + tile; tile = 64 positions c.
template <bool kToPacked>
__global__ __launch_bounds__(kDfBlock)
void nerf_deform_repack_kernel(DfTables tabs, float* __restrict__ packed, int T, int R, int tiles) {
  __shared__ float s_tile[kDfF][kDfF + 1];                       // [f][c], odd pitch
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x % tiles;
  const int y = (blockIdx.x / tiles) % T;
  const int ij = blockIdx.x / (tiles * T);                       // < 9: the grid is 9 * T * tiles
  const int c0 = tile * 64;
  float* __restrict__ tab = tabs.t[ij / 3] + ((size_t)(ij % 3) * kDfF * T + y) * R;       // + f * T * R + c
  float* __restrict__ pk = packed + (((size_t)ij * T + y) * R) * kDfF;                     // + c * 64 + f
  if (kToPacked) {
    if (c0 + lane < R)
      for (int f = wave; f < kDfF; f += kDfBlock / 64) s_tile[f][lane] = tab[(size_t)f * T * R + c0 + lane];
    __syncthreads();
    for (int c = wave; c < 64 && c0 + c < R; c += kDfBlock / 64) pk[(size_t)(c0 + c) * kDfF + lane] = s_tile[lane][c];
  } else {
    for (int c = wave; c < 64 && c0 + c < R; c += kDfBlock / 64) s_tile[lane][c] = pk[(size_t)(c0 + c) * kDfF + lane];
    __syncthreads();
    if (c0 + lane < R)
      for (int f = wave; f < kDfF; f += kDfBlock / 64) tab[(size_t)f * T * R + c0 + lane] = s_tile[f][lane];
  }
}

bool df_misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

// F == 64, T >= 2, R >= 2, 9 * T * R * 64 <= 2^31 - 1 -> the floats of `packed`, or -1
int64_t df_packed_floats(int32_t F, int32_t T, int32_t R) {
  if (F != kDfF || T < 2 || R < 2) return -1;
  const int64_t n = 9 * (int64_t)T * (int64_t)R * kDfF;
  return n > 0x7fffffffLL ? -1 : n;
}

int df_check_domain(const char* entry, int32_t F, int32_t T, int32_t R) {
  if (df_packed_floats(F, T, R) < 0)
    return fail(NERF_ERR_INVALID_ARG, "%s: needs n_channels == 64, n_frames >= 2, reso >= 2 and 9 * n_frames * reso * 64 <= 2^31 - 1", entry);
  return NERF_OK;
}

// the sizes and the pointers the forward and the backward share
int df_check_rows(const char* entry, const float* x, const float* time, const int32_t* index, int64_t n_rows, int64_t n_rays,
                  int32_t n_samples, const float* packed, int32_t F, int32_t T, int32_t R) {
  const int rc = df_check_domain(entry, F, T, R);
  if (rc) return rc;
  if (n_samples < 1 || n_samples > kDfMaxSamples) return fail(NERF_ERR_INVALID_ARG, "%s: n_samples must be in [1, 192]", entry);
  if (n_rays <= 0 || n_rays > 0x7fffffffLL / n_samples)
    return fail(NERF_ERR_INVALID_ARG, "%s: n_rays must be positive and n_rays * n_samples at most 2^31 - 1", entry);
  if (n_rows <= 0 || n_rows > n_rays * n_samples)
    return fail(NERF_ERR_INVALID_ARG, "%s: n_rows must be in [1, n_rays * n_samples]", entry);
  if (!x || !time || !packed) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (df_misaligned(x, 4) || df_misaligned(time, 4) || df_misaligned(index, 4) || df_misaligned(packed, 256))
    return fail(NERF_ERR_INVALID_ARG, "%s: x, time and index must be aligned to 4 bytes, packed to 256", entry);
  return NERF_OK;
}

DfArgs df_args(const float* x, const float* time, const int32_t* index, int64_t n_rows, int64_t n_rays, int32_t n_samples,
               const float* packed, int32_t T, int32_t R) {
  DfArgs a;
  a.x = x; a.time = time; a.index = index; a.n_rows = (uint32_t)n_rows; a.n_points = (uint32_t)(n_rays * n_samples);
  a.n_samples = (uint32_t)n_samples; a.packed = packed; a.T = T; a.R = R;
  return a;
}

inline dim3 df_grid(int64_t n_rows) { return dim3((unsigned)((n_rows + kDfBlock / 64 - 1) / (kDfBlock / 64))); }

}  // namespace

extern "C" {

int64_t nerf_deform_packed_bytes(int32_t n_channels, int32_t n_frames, int32_t reso) {
  const int64_t n = df_packed_floats(n_channels, n_frames, reso);
  return n < 0 ? -1 : n * 4;
}

int64_t nerf_deform_table_bytes(int32_t n_channels, int32_t n_frames, int32_t reso) {
  const int64_t n = df_packed_floats(n_channels, n_frames, reso);
  return n < 0 ? -1 : n / 3 * 4;
}

int32_t nerf_deform_pack(const float* const feat[3], int32_t n_channels, int32_t n_frames, int32_t reso, float* packed, void* stream) {
  const char* entry = "nerf_deform_pack";
  const int rc = df_check_domain(entry, n_channels, n_frames, reso);
  if (rc) return rc;
  if (!feat || !feat[0] || !feat[1] || !feat[2] || !packed) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (df_misaligned(feat[0], 4) || df_misaligned(feat[1], 4) || df_misaligned(feat[2], 4) || df_misaligned(packed, 256))
    return fail(NERF_ERR_INVALID_ARG, "%s: the tables must be aligned to 4 bytes, packed to 256", entry);
  DfTables tabs;
  for (int i = 0; i < 3; ++i) tabs.t[i] = const_cast<float*>(feat[i]);      // (read only in this direction)
  const int tiles = (reso + 63) / 64;
  return NERF_LAUNCH(nerf_deform_repack_kernel<true>, dim3((unsigned)(9 * n_frames * tiles)), dim3(kDfBlock), (hipStream_t)stream, tabs,
                     packed, (int)n_frames, (int)reso, tiles);
}

int32_t nerf_deform_unpack_grad(const float* g_packed, int32_t n_channels, int32_t n_frames, int32_t reso, float* const g_feat[3],
                                void* stream) {
  const char* entry = "nerf_deform_unpack_grad";
  const int rc = df_check_domain(entry, n_channels, n_frames, reso);
  if (rc) return rc;
  if (!g_feat || !g_feat[0] || !g_feat[1] || !g_feat[2] || !g_packed) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (df_misaligned(g_feat[0], 4) || df_misaligned(g_feat[1], 4) || df_misaligned(g_feat[2], 4) || df_misaligned(g_packed, 256))
    return fail(NERF_ERR_INVALID_ARG, "%s: the tables must be aligned to 4 bytes, g_packed to 256", entry);
  DfTables tabs;
  for (int i = 0; i < 3; ++i) tabs.t[i] = g_feat[i];
  const int tiles = (reso + 63) / 64;
  return NERF_LAUNCH(nerf_deform_repack_kernel<false>, dim3((unsigned)(9 * n_frames * tiles)), dim3(kDfBlock), (hipStream_t)stream, tabs,
                     const_cast<float*>(g_packed), (int)n_frames, (int)reso, tiles);
}

int32_t nerf_deform_forward(const float* x, const float* time, const int32_t* index, int64_t n_rows, int64_t n_rays, int32_t n_samples,
                            const float* packed, int32_t n_channels, int32_t n_frames, int32_t reso, float* x_warped, float* delta,
                            void* stream) {
  const char* entry = "nerf_deform_forward";
  const int rc = df_check_rows(entry, x, time, index, n_rows, n_rays, n_samples, packed, n_channels, n_frames, reso);
  if (rc) return rc;
  if (!x_warped && !delta) return fail(NERF_ERR_INVALID_ARG, "%s: one of x_warped and delta must be given", entry);
  if (df_misaligned(x_warped, 4) || df_misaligned(delta, 4))
    return fail(NERF_ERR_INVALID_ARG, "%s: x_warped and delta must be aligned to 4 bytes", entry);
  return NERF_LAUNCH(nerf_deform_forward_kernel, df_grid(n_rows), dim3(kDfBlock), (hipStream_t)stream,
                     df_args(x, time, index, n_rows, n_rays, n_samples, packed, n_frames, reso), x_warped, delta);
}

int32_t nerf_deform_backward(const float* x, const float* time, const int32_t* index, int64_t n_rows, int64_t n_rays,
                             int32_t n_samples, const float* packed, int32_t n_channels, int32_t n_frames, int32_t reso,
                             const float* g_x_warped, const float* g_delta, float* g_packed, void* stream) {
  const char* entry = "nerf_deform_backward";
  const int rc = df_check_rows(entry, x, time, index, n_rows, n_rays, n_samples, packed, n_channels, n_frames, reso);
  if (rc) return rc;
  if (!g_packed) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!g_x_warped && !g_delta) return fail(NERF_ERR_INVALID_ARG, "%s: one of g_x_warped and g_delta must be given", entry);
  if (df_misaligned(g_x_warped, 4) || df_misaligned(g_delta, 4) || df_misaligned(g_packed, 256))
    return fail(NERF_ERR_INVALID_ARG, "%s: g_x_warped and g_delta must be aligned to 4 bytes, g_packed to 256", entry);
  return NERF_LAUNCH(nerf_deform_backward_kernel, df_grid(n_rows), dim3(kDfBlock), (hipStream_t)stream,
                     df_args(x, time, index, n_rows, n_rays, n_samples, packed, n_frames, reso), g_x_warped, g_delta, g_packed);
}

}  // extern "C"
