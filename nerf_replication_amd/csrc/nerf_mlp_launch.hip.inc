// Every launch of an MLP forward kernel: the instance families per precision, launch_mlp, the ray-mode front forward_rays, and the
// inference and SAVE (training forward) entries.
// Needs, ahead of it, the forward kernel files (nerf_mlp_f32 / f16 / f16s / f32x.hip.inc) with the split-fp16 instance list
// (nerf_kernels_x.inst.inc).
#include "nerf_host.h"
#include "nerf_mlp_common.h"

namespace {

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

// ------------------------------------------------------------------------------------ dead k-step skipping (fp32 inference instances)
// On unless NERF_DEAD_KSTEP_SKIP=0: with 0 the kernel issues every MFMA (the A/B reference of the bit-identity tests, and the
// price of the decision by itself).  Read per launch, like the switch above.
int dead_kstep_skip_wanted() {
  const char* env = getenv("NERF_DEAD_KSTEP_SKIP");
  return !(env && env[0] == '0');
}

// Leading dead groups (gemm_tiles `prefix`): on unless NERF_DEAD_GROUP_SKIP=0, which leaves the row decisions above alone -- the
// A/B switch of this path by itself.  NERF_DEAD_KSTEP_SKIP=0 switches both off.
int dead_group_skip_wanted() {
  const char* env = getenv("NERF_DEAD_GROUP_SKIP");
  return dead_kstep_skip_wanted() && !(env && env[0] == '0');
}

// ------------------------------------------------------------------------------------ tile shape (fp32 inference ray instances)
// NERF_TILE_RAYS = 1, 2, 4, 8, 16 or 32: rays per 32-point tile (MlpArgs::tile_rays_log2), read per launch.  Unset (or any other
// value): the caller's default -- render_frame's dense launches ask for kRenderTileRaysLog2, the direct entries for one-ray tiles.
constexpr int kRenderTileRaysLog2 = 3;
int tile_rays_log2_wanted(int dflt) {
  const char* env = getenv("NERF_TILE_RAYS");
  if (!env) return dflt;
  for (int lg = 0; lg <= 5; ++lg) {
    char want[4];
    snprintf(want, sizeof want, "%d", 1 << lg);
    if (!strcmp(env, want)) return lg;
  }
  return dflt;
}

}  // namespace

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
  a.skip_dead_ksteps = dead_kstep_skip_wanted();
  a.skip_dead_groups = dead_group_skip_wanted();
  if (f->persistent) return launch(f->name, k, dim3(persistent_blocks(a.n_points, f->wg_pts)), dim3(f->threads), st, a);
  // shaped tiles (forward_rays): ceil(n_rays / R) ray groups of n_samples / (32 >> lg) tiles, i.e. the points of whole groups
  long long grid_pts = a.n_points;
  if (a.tile_rays_log2) {
    const long long R = 1LL << a.tile_rays_log2;
    grid_pts = (a.n_points / a.n_samples + R - 1) / R * R * a.n_samples;
  }
  const long long blocks = (grid_pts + f->wg_pts - 1) / f->wg_pts;
  if (blocks > 0x7fffffffLL) return fail(NERF_ERR_INVALID_ARG, "%s: too many points for one launch", entry);
  return launch(f->name, k, dim3((unsigned)blocks), dim3(f->threads), st, a);
}

// The ray-mode forward entries.  for_compositing: `raw` only ever reaches nerf_composite, where the colours of zero-density
// samples are multiplied by exactly 0, so tiles without density skip the colour branch (DSKIP).  want_save: the training forward.
// index / count (masked): rows of index[j] at slot j, `raw` at the id (every instance honours both).
static int forward_rays(const char* entry, const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                        int32_t n_samples, const void* packed, float* raw, bool want_save, float* save, bool density_only,
                        bool for_compositing, int32_t precision, void* stream, const int* index = nullptr, const int* count = nullptr,
                        int tile_rays_log2 = 0) {
  if (n_rays < 0 || n_samples <= 0 || t_ray_stride < 0) return fail(NERF_ERR_INVALID_ARG, "%s: bad size", entry);
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !tvals || !packed || !raw || (want_save && !save)) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  MlpArgs a{};
  a.rays_o = rays_o; a.rays_d = rays_d; a.tvals = tvals; a.t_ray_stride = t_ray_stride;
  a.n_points = n_rays * n_samples; a.n_samples = n_samples; a.packed = (const float*)packed; a.raw = raw; a.save = save;
  a.density_only = density_only; a.skip_dead_colour = for_compositing;
  a.index = index; a.count = count;
  // tile shape: the fp32 inference instances without a list, and only where a tile's samples divide the ray
  const int lg = tile_rays_log2_wanted(tile_rays_log2);
  a.tile_rays_log2 = precision == NERF_PREC_F32 && !index && !want_save && n_samples % (32 >> lg) == 0 ? lg : 0;
  if (want_save) {
    // without dead-tile skipping in the backward pass every row must exist: fall back to the full store (the SAME helper decides
    // for the backward pass).  The buffer is stamped with what is done here: 1 = the rows of density-free tiles are NOT stored
    a.skip_dead_colour = for_compositing && dead_tile_list_available(a.n_points, precision);
    if (hipMemsetAsync(save + TrainSave::off_stamp(a.n_points), a.skip_dead_colour ? 0x01 : 0x00, 4 * sizeof(float), (hipStream_t)stream) != hipSuccess)
      return fail(NERF_ERR_HIP, "%s: memset failed", entry);
  }
  return launch_mlp(a, true, want_save, precision, (hipStream_t)stream, entry);
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

}  // extern "C"
