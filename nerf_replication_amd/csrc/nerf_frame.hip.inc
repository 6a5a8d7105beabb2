// One frame, block by block through the four stages (coarse MLP, fine sampler, fine MLP, compositing): the block workspace,
// render_frame, and the entries nerf_render_forward / nerf_render_forward_stochastic with their workspace sizes.
// Needs, ahead of it, nerf_sampling.hip.inc (nerf_compact_kernel, nerf_last_sample_index_kernel) and
// nerf_mlp_launch.hip.inc (forward_rays); nerf_occupancy.hip.inc comes behind it (nerf_render_forward_occupancy calls render_frame).
#include "nerf_host.h"

namespace {

// evaluated += the length of the list a pass just ran on (count), or `all` for a pass without a list.  One thread; the launches of
// a frame are ordered by the stream, so nothing here is atomic.
__global__ void nerf_occupancy_tally_kernel(const int* __restrict__ count, long long all, long long* __restrict__ evaluated) {
  *evaluated += count ? (long long)*count : all;
}

}  // namespace

extern "C" {

// Ray blocks.  nerf_render_forward walks a frame in blocks of kRenderBlockRays rays (the four stages per block, same stream): the
// intermediates -- raw_coarse, t_sorted, raw_fine: 4864 B per ray -- belong to ONE block, so the workspace is bounded (5.1 GB) whatever
// the frame (round 2: 12.5 GB at 1600x1600, growing with the frame).  Rays are independent: the image is bit-identical to the one-block
// render (tests).  The block is LARGE on purpose: with 65 536-ray blocks (320 MB, Infinity-Cache-resident intermediates) the fp32
// frame lost 0.2 % and the fp16 frame 5 % (134.7 -> 141.4 ms at 800x800) -- every block pays the persistent kernels' pipeline fill and
// tail, and the far-plane guard's launch (one point per ray) fills 2 tiles per CU -- while nothing is gained from the cache
// residency: the MLP launches are matrix-bound and HBM sits at < 1 % of its bandwidth either way.  NERF_RENDER_BLOCK_RAYS in the
// environment overrides the block size (A/B, tests).
static constexpr int64_t kRenderBlockRays = 1 << 20;
static int64_t render_block_rays() {
  const char* env = getenv("NERF_RENDER_BLOCK_RAYS");
  // capped at the rays whose 192 point ids fit in int32: a larger block would switch the fp16 far-plane guard off (render_frame)
  constexpr long long kMax = 0x7fffffff / (NERF_N_SAMPLES + NERF_N_IMPORTANCE);
  if (env) { const long long v = atoll(env); if (v >= 64) return (int64_t)(v < kMax ? v : kMax); }
  return kRenderBlockRays;
}

// The workspace of one block of `n_rays` rays, carved in this order, every piece 256-byte aligned.  index / count: with fast_sampling
// the compacted ids of the valid merged samples and their number (and, once that list is consumed, the guard's), otherwise the
// last-sample ids of the fp16 far-plane guard and their number.  t_jit: the jittered coarse depths [n,64] of a stochastic render.  occupancy (nerf_render_forward_occupancy): the
// fine pass may be listed without fast_sampling too, and the coarse pass gets a mask [n,64] and an id list of its own behind.
struct RenderWorkspace {
  float* raw_c; float* t_sorted = nullptr; float* raw_f = nullptr; uint8_t* valid = nullptr; int* index; int* count; float* t_jit = nullptr;
  uint8_t* valid_c = nullptr; int* index_c = nullptr;
  int64_t bytes;
  RenderWorkspace(void* base, int64_t n_rays, int32_t n_importance, int32_t fast_sampling, bool stochastic, bool occupancy = false) {
    Carver c(base);
    const int64_t S = NERF_N_SAMPLES + NERF_N_IMPORTANCE;
    raw_c = c.take<float>(n_rays * NERF_N_SAMPLES * 4);
    if (n_importance) {
      t_sorted = c.take<float>(n_rays * S);
      raw_f = c.take<float>(n_rays * S * 4);
    }
    if (n_importance && (fast_sampling || occupancy)) {
      valid = c.take<uint8_t>(n_rays * S);
      index = c.take<int>(n_rays * S);
    } else {
      index = c.take<int>(n_rays);
    }
    count = c.take<int>(1);
    if (stochastic) t_jit = c.take<float>(n_rays * NERF_N_SAMPLES);
    if (occupancy) {
      valid_c = c.take<uint8_t>(n_rays * NERF_N_SAMPLES);
      index_c = c.take<int>(n_rays * NERF_N_SAMPLES);
    }
    bytes = c.bytes();
  }
};
static int64_t render_workspace_bytes(int64_t n_rays_frame, int32_t n_importance, int32_t fast_sampling, bool stochastic,
                                      bool occupancy = false) {
  if (n_rays_frame < 0) return -1;
  const int64_t n_rays = n_rays_frame < render_block_rays() ? n_rays_frame : render_block_rays();
  return RenderWorkspace(nullptr, n_rays, n_importance, fast_sampling, stochastic, occupancy).bytes;
}

// Occupancy culling of a frame (nerf_render_forward_occupancy, csrc/nerf_occupancy.hip.inc): the bitfields of the coarse and the fine
// pass (each nullable: that pass runs on every sample), the lookup frame, and the DEVICE int64[2] that takes the numbers of coarse /
// fine points evaluated (nullable).
struct RenderOccupancy {
  const uint32_t* coarse; const uint32_t* fine;
  int32_t dims[3]; float box_min[3], inv_step[3];
  long long* evaluated;
};
// render_frame's tally of the points a pass evaluated
static int occupancy_tally(const int* count, long long all, long long* evaluated, hipStream_t st) {
  return NERF_LAUNCH(nerf_occupancy_tally_kernel, dim3(1), dim3(1), st, count, all, evaluated);
}
int64_t nerf_render_workspace_bytes(int64_t n_rays_frame, int32_t n_importance, int32_t fast_sampling) {
  return render_workspace_bytes(n_rays_frame, n_importance, fast_sampling, false);
}
int64_t nerf_render_stochastic_workspace_bytes(int64_t n_rays_frame, int32_t n_importance) {
  return render_workspace_bytes(n_rays_frame, n_importance, 0, true);
}

// One frame, block by block through the four stages.  jitter / u_rays (stochastic render: task == "train", no grad) give every ray
// its own coarse depths (nerf_stratified_samples of the block, stride 64) and its own u (stride 128); without them the shared
// tables go through with stride 0, and nerf_sample_fine_rays then launches nerf_sample_fine_kernel.
static int32_t render_frame(const char* entry, const float* rays_o, const float* rays_d, int64_t n_rays, const void* packed_coarse,
                            const void* packed_fine, const float* t_coarse, const float* u, const float* jitter, const float* u_rays,
                            bool stochastic, int32_t n_importance, int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                            float weights_threshold, void* workspace, int64_t workspace_bytes, float* rgb, float* depth, void* stream,
                            const RenderOccupancy* occ = nullptr) {
  if (n_rays < 0) return fail(NERF_ERR_INVALID_ARG, "%s: bad size", entry);
  if (n_importance != 0 && n_importance != NERF_N_IMPORTANCE)
    return fail(NERF_ERR_INVALID_ARG, "%s: n_importance must be 0 or 128", entry);
  if (n_rays == 0) return NERF_OK;
  if (!rays_o || !rays_d || !packed_coarse || !t_coarse || !rgb || !depth || !workspace ||
      (n_importance && (!packed_fine || !u)))
    return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (workspace_bytes < render_workspace_bytes(n_rays, n_importance, fast_sampling, stochastic, occ != nullptr))
    return fail(NERF_ERR_WORKSPACE, "%s: workspace too small", entry);
  // the masked fine pass addresses (ray, sample) pairs by 32-bit ids (nerf_compact_kernel, MlpArgs::index)
  const int64_t S = NERF_N_SAMPLES + NERF_N_IMPORTANCE;
  if (fast_sampling && n_importance && n_rays > (int64_t)0x7fffffff / S)
    return fail(NERF_ERR_INVALID_ARG, "%s: fast_sampling handles at most 11 184 810 rays per call "
                                      "(n_rays * 192 point ids must fit in int32): split the frame", entry);
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = render_block_rays();
  for (int64_t r0 = 0; r0 < n_rays; r0 += B) {
    const int64_t nb = n_rays - r0 < B ? n_rays - r0 : B;
    const float* o = rays_o + 3 * r0;
    const float* d = rays_d + 3 * r0;
    float* rgb_b = rgb + 3 * r0;
    float* depth_b = depth + r0;
    const RenderWorkspace w(workspace, nb, n_importance, fast_sampling, stochastic, occ != nullptr);
    // A pass on a list: the ids with valid != 0 compacted (unordered: `raw` is written by id), `raw` zero-filled -- an unlisted
    // sample keeps raw = 0, and compositing and the sampler both apply relu(sigma), so that is exact wherever its true sigma <= 0
    auto list_pass = [&](const uint8_t* valid, long long np, int* index, float* raw) -> int {
      if (hipMemsetAsync(w.count, 0, sizeof(int), st) != hipSuccess ||
          hipMemsetAsync(raw, 0, (size_t)(np * 4 * (int64_t)sizeof(float)), st) != hipSuccess)
        return fail(NERF_ERR_HIP, "%s: memset failed", entry);
      return NERF_LAUNCH(nerf_compact_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), st, valid, np, index, w.count);
    };
    // (occupancy) the points a pass evaluated: the length of its list, or all of them
    auto tally = [&](int pass, bool listed, long long all) -> int {
      return occ && occ->evaluated ? occupancy_tally(listed ? w.count : nullptr, all, occ->evaluated + pass, st) : NERF_OK;
    };
    const float* tc = t_coarse;
    int64_t tcs = 0;
    int rc;
    if (jitter) {
      rc = nerf_stratified_samples(t_coarse, jitter + NERF_N_SAMPLES * r0, nb, w.t_jit, stream);
      if (rc) return rc;
      tc = w.t_jit; tcs = NERF_N_SAMPLES;
    }
    // hierarchical render: the coarse network only places the fine samples -- nothing but its sigma is read
    // (volume_renderer.py:335; the returned rgb/depth come from the fine outputs, :414-437), so the coarse pass stops after
    // the sigma head.  With n_importance == 0 the coarse outputs ARE the frame and the full network runs.
    const bool cull_c = occ && occ->coarse;
    if (cull_c) {
      rc = nerf_occupancy_mark(o, d, tc, tcs, nb, NERF_N_SAMPLES, occ->coarse, occ->dims, occ->box_min, occ->inv_step, 0, w.valid_c, stream);
      if (rc) return rc;
      rc = list_pass(w.valid_c, nb * NERF_N_SAMPLES, w.index_c, w.raw_c);
      if (rc) return rc;
    }
    // fp16 with fast_sampling: the coarse sigma also DECIDES -- the ESS / ERT mask compares the coarse weights with thresholds, and a
    // weight that crosses one keeps or drops all the fine samples in front of a surface.  With the fp16 coarse sigma the masked render
    // stood at 41-47 dB against the masked f32 render where the plain one stands at 54-58, single rays 1.1 off in depth; so the
    // density pass of that combination runs on the split-fp16 stream behind the packed model (fp32-accurate, as the guard below):
    // 54-88 dB, no ray above 0.27.  It costs the masked fp16 frame 91.5 -> 151.6 ms at 800x800 (LAB_NOTEBOOK).
    const bool fp16 = precision == NERF_PREC_F16 || precision == NERF_PREC_F16S;
    const bool exact_coarse = fp16 && fast_sampling && n_importance;
    rc = forward_rays(entry, o, d, tc, tcs, nb, NERF_N_SAMPLES, exact_coarse ? (const char*)packed_coarse + nerf::kF16PackedBytes : packed_coarse,
                      w.raw_c, false, nullptr, n_importance != 0, false, exact_coarse ? NERF_PREC_F32X : precision, stream,
                      cull_c ? w.index_c : nullptr, cull_c ? w.count : nullptr, kRenderTileRaysLog2);
    if (rc) return rc;
    rc = tally(0, cull_c, nb * NERF_N_SAMPLES);
    if (rc) return rc;
    // fp16 far-plane guard.  The last sample of a ray has delta = 1e10 (volume_renderer.py:85-86): ANY sigma > 0 there makes alpha = 1, so
    // an fp16 rounding that flips the sign of a sigma within 1e-2 of zero turns a background ray into a full far-plane hit (round 2:
    // single rays off by 0.64 in rgb and 6.0 in depth, which alone set the fp16 PSNR).  Every other sample's alpha moves by
    // |d sigma| * delta ~ 1e-4.  So the fp16 precisions re-evaluate exactly that sample of every ray (0.5 % of the points) with the
    // split-fp16 stream that rides behind their packed model: fp32-accurate sigma and colour where it matters, ~1.5 % of the frame.
    const bool guard = fp16 && nb <= (int64_t)0x7fffffff / S;
    auto far_plane_guard = [&](const float* tvals, int64_t stride, int32_t S_, const void* packed_f16, float* raw) -> int {
      if (const int r2 = NERF_LAUNCH(nerf_last_sample_index_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), st, w.index, w.count,
                                     (long long)nb, S_)) return r2;
      return forward_rays(entry, o, d, tvals, stride, nb, S_, (const char*)packed_f16 + nerf::kF16PackedBytes, raw, false, nullptr, false,
                          false, NERF_PREC_F32X, stream, w.index, w.count);
    };
    if (n_importance == 0) {
      if (guard) {
        rc = far_plane_guard(tc, tcs, NERF_N_SAMPLES, packed_coarse, w.raw_c);
        if (rc) return rc;
      }
      rc = nerf_composite(w.raw_c, tc, tcs, nb, NERF_N_SAMPLES, white_bkgd, rgb_b, depth_b, nullptr, stream);
      if (rc) return rc;
      continue;
    }
    // fast_sampling, ESS/ERT (volume_renderer.py:359-369, network.py:207-253): the sampler also marks the valid merged samples
    rc = nerf_sample_fine_rays(w.raw_c, tc, tcs, u_rays ? u_rays + NERF_N_IMPORTANCE * r0 : u, u_rays ? NERF_N_IMPORTANCE : 0, nb, w.t_sorted,
                               nullptr, fast_sampling ? w.valid : nullptr, fast_sampling ? weights_threshold : 0.f, fast_sampling ? 0.45f : 0.f,
                               stream);
    if (rc) return rc;
    const bool cull_f = occ && occ->fine;
    if (cull_f) {
      rc = nerf_occupancy_mark(o, d, w.t_sorted, S, nb, (int32_t)S, occ->fine, occ->dims, occ->box_min, occ->inv_step, fast_sampling != 0, w.valid,
                               stream);
      if (rc) return rc;
    }
    if (!fast_sampling && !cull_f) {
      rc = forward_rays(entry, o, d, w.t_sorted, S, nb, (int32_t)S, packed_fine, w.raw_f, false, nullptr, false, true, precision, stream, nullptr,
                        nullptr, kRenderTileRaysLog2);
      if (rc) return rc;
      if (guard) {
        rc = far_plane_guard(w.t_sorted, S, (int32_t)S, packed_fine, w.raw_f);
        if (rc) return rc;
      }
    } else {
      // only the valid merged samples go through the fine network; the others keep raw = 0 (sigma 0 -> weight 0)
      rc = list_pass(w.valid, nb * S, w.index, w.raw_f);
      if (rc) return rc;
      rc = forward_rays(entry, o, d, w.t_sorted, S, nb, (int32_t)S, packed_fine, w.raw_f, false, nullptr, false, true, precision, stream,
                        w.index, w.count);
      if (rc) return rc;
    }
    rc = tally(1, fast_sampling || cull_f, nb * S);
    if (rc) return rc;
    // the guard of the masked fine pass.  Under fast_sampling alone the last merged sample of every ray is its coarse far sample,
    // and coarse samples are always valid: it is in the list, the fp16 network has just written it, and the exposure is the plain
    // branch's.  The list has been consumed (the forward and the tally are enqueued), so w.index / w.count are free for the guard's
    // ids.  With a fine occupancy field a last sample may be unlisted and must keep raw = 0: that combination stays as it is (the
    // package refuses fp16 with occupancy, modes.py).
    if (guard && fast_sampling && !cull_f) {
      rc = far_plane_guard(w.t_sorted, S, (int32_t)S, packed_fine, w.raw_f);
      if (rc) return rc;
    }
    rc = nerf_composite(w.raw_f, w.t_sorted, S, nb, (int32_t)S, white_bkgd, rgb_b, depth_b, nullptr, stream);
    if (rc) return rc;
  }
  return NERF_OK;
}

int32_t nerf_render_forward(const float* rays_o, const float* rays_d, int64_t n_rays,
                            const void* packed_coarse, const void* packed_fine,
                            const float* t_coarse, const float* u, int32_t n_importance,
                            int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                            float weights_threshold, void* workspace,
                            int64_t workspace_bytes, float* rgb, float* depth, void* stream) {
  return render_frame("nerf_render_forward", rays_o, rays_d, n_rays, packed_coarse, packed_fine, t_coarse, u, nullptr, nullptr, false,
                      n_importance, white_bkgd, precision, fast_sampling, weights_threshold, workspace, workspace_bytes, rgb, depth, stream);
}

int32_t nerf_render_forward_stochastic(const float* rays_o, const float* rays_d, int64_t n_rays,
                                       const void* packed_coarse, const void* packed_fine,
                                       const float* t_coarse, const float* u, const float* jitter, const float* u_rays,
                                       int32_t n_importance, int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                                       float weights_threshold, void* workspace, int64_t workspace_bytes,
                                       float* rgb, float* depth, void* stream) {
  if (precision != NERF_PREC_F32 && precision != NERF_PREC_F32X)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_render_forward_stochastic: precision must be f32 or f32x");
  if (fast_sampling) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_render_forward_stochastic: fast_sampling is not supported");
  return render_frame("nerf_render_forward_stochastic", rays_o, rays_d, n_rays, packed_coarse, packed_fine, t_coarse, u, jitter, u_rays,
                      true, n_importance, white_bkgd, precision, 0, weights_threshold, workspace, workspace_bytes, rgb, depth, stream);
}

}  // extern "C"
