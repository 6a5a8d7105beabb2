/* nerf_mi355x.h -- C ABI of libnerf_mi355x.so: the NeRF volume-rendering hot path on MI355X (gfx950).
 *
 * The reference (rkin100g/Nerf-Replication) is pure Python on PyTorch ATen ops: there is no native
 * interface on this path to mirror.  The entry points below are therefore
 * what a reference-side binding (ctypes) would call from inside the reference's
 * own plugin surface:
 *     src/models/nerf/renderer/volume_renderer.py:290-432   Renderer.render
 *     src/models/nerf/network.py:199-258                    Network.forward
 * Each function cites the reference lines whose arithmetic it replaces.
 *
 * Conventions: every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated
 * otherwise; inputs are borrowed, outputs are caller-allocated; `stream` is a hipStream_t (NULL =
 * default stream); calls only enqueue work (no host sync, graph-capturable); the return value is 0
 * on success or a negative nerf_status, never an exception; nerf_last_error() gives the message of
 * the calling thread's last failure.  n_rays == 0 is a successful no-op everywhere.
 *
 * The library allocates no device memory and keeps no state between calls beyond the thread-local
 * error text (and the device's compute-unit count, read once).  The fp32 kernels evaluate the colour branch on
 * feature_linear folded into the views layer; that fold is part of the packed fp32 model
 * (nerf_pack_model writes it behind the weight stream) and is as fresh as the pack.
 */
#ifndef NERF_MI355X_H
#define NERF_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version 3.  Contracts that changed since version 2 (entry names and signatures did not):
 *   - the packed fp32 model carries the fold of feature_linear into the views layer behind its weight stream:
 *     nerf_packed_model_bytes(NERF_PREC_F32) grew, a version-2 packed model lacks the fold and a version-2-sized buffer is too
 *     small for nerf_pack_model; `packed` must be 256-byte aligned.
 * Version 2 (round 3).  Contracts that changed since version 1:
 *   - the TrainSave / TrainGrad buffers (nerf_train_save_floats / nerf_train_grad_floats) hold pad32(P) rows per region, with the
 *     ReLU sign-bit blocks, the live-tile flags / list / count and a "rows skipped" stamp appended;
 *     nerf_mlp_backward (both precisions) takes its ReLU masks from those sign bits (written by the SAVE forwards only);
 *   - both precisions: the density entries skip the colour branch (its rows and sign bits are not stored / not read), and lanes
 *     past the last point write the pad32 padding rows of every region;
 *   - with dead-tile skipping (default; NERF_DEAD_TILE_SKIP=0 in the environment disables it) the g_z rows of tiles whose incoming
 *     gradient is zero throughout are left unwritten in `gsave` (point mode zero-fills the g_zv region, which
 *     nerf_viewdirs_backward sums over; ray mode leaves them unwritten, and nerf_rays_viewdirs_backward skips them by their flag);
 *   - nerf_mlp_forward_rays_save_for_compositing may omit the rows of density-free tiles; it stamps the buffer, and a backward pass
 *     that runs without the live-tile list on such a buffer poisons grads[alpha_linear.bias] with NaN instead of reading them;
 *   - nerf_composite_backward refuses more than 192 samples per ray. */
#define NERF_ABI_VERSION 3

enum nerf_status {
  NERF_OK = 0,
  NERF_ERR_INVALID_ARG = -1,   /* null pointer, negative size, unsupported sample counts */
  NERF_ERR_WORKSPACE = -2,     /* workspace too small */
  NERF_ERR_HIP = -3,           /* a HIP runtime call or kernel launch failed */
  NERF_ERR_UNSUPPORTED = -4    /* precision / mode not built */
};

enum nerf_precision {
  NERF_PREC_F32 = 0,           /* exact fp32: v_mfma_f32_32x32x2_f32 (the parity path) */
  NERF_PREC_F16 = 1,           /* fp16 activations+weights, fp32 accumulate: v_mfma_f32_32x32x16_f16
                                  (BASELINE config 5; PSNR-level tolerance, not the parity path) */
  NERF_PREC_F32X = 2,          /* fp32-accurate on the fp16 matrix cores: every operand split into hi + 2^-11 lo
                                  fp16 parts, 3 MFMAs per product, fp32 accumulate (~2^-22 operand error) */
  NERF_PREC_F16S = 3           /* NERF_PREC_F16's arithmetic on the other MFMA shape, v_mfma_f32_16x16x32_f16 (same operands and
                                  accumulation width; only the order of the fp32 partial sums differs); its own packed layout */
};

/* Renderer constants the reference effectively hard-codes (volume_renderer.py:14-24). */
#define NERF_N_SAMPLES 64
#define NERF_N_IMPORTANCE 128

int32_t nerf_abi_version(void);

/* Build self-description: 0 for a product build.  Timing experiments (tools/ab_bench.py) compile kernels with
   switches that change their numerics; such a library only builds with -DNERF_TIMING_BUILD and reports it here.
   A binder must refuse a non-zero value (nerf_replication_amd/_lib.py does). */
enum nerf_build_flag { NERF_BUILD_TIMING = 1, NERF_BUILD_WRONG_NUMERICS = 2 };
int32_t nerf_build_flags(void);
const char* nerf_last_error(void);

/* Size in bytes of one packed sub-model (coarse or fine) for a precision; -1 if unknown.  A packed model is a caller-owned
 * buffer of this size, 256-byte aligned (a torch allocation is). */
int64_t nerf_packed_model_bytes(int32_t precision);

/* Permute the 24 parameter tensors of one NeRF sub-model into the kernel's weight stream
 * (csrc/nerf_layout.h).  `params` is a HOST array of 24 DEVICE pointers in the reference's
 * state_dict order (network.py:22-47): pts_linears.0..7 {weight,bias}, views_linears.0,
 * feature_linear, alpha_linear, rgb_linear; weights are nn.Linear [out,in] row-major.
 * Runs on the device; call again whenever the parameters change (e.g. after an optimizer step). */
int32_t nerf_pack_model(const float* const params[24], void* packed, int32_t precision, void* stream);

/* Positional encoding alone: x [n,3] -> out [n, 3+6*n_freqs] in the reference's channel order.
 * Replaces freq.py:31-32 (Encoder.embed); n_freqs is 10 (xyz) or 4 (view dir). Uses the same
 * device sincos as the fused MLP; exposed for parity tests. */
int32_t nerf_positional_encoding(const float* x, int64_t n, int32_t n_freqs, float* out, void* stream);

/* Network.forward(inputs[n,s,3], viewdirs[n,3], valid_mask=None, model) -> raw [n,s,4] = (r,g,b,sigma)
 * pre-activation.  Replaces network.py:216-256: PE of points and directions, the batchify(512) loop
 * over NeRF.forward (network.py:49-74), and the reshape.  `packed` selects coarse or fine model. */
int32_t nerf_mlp_forward(const float* pts, const float* viewdirs, int64_t n_rays, int32_t n_samples,
                         const void* packed, float* raw, int32_t precision, void* stream);

/* Same network on points generated on the fly: pts = rays_o + rays_d * t (volume_renderer.py:63,
 * :267), viewdirs = rays_d / ||rays_d|| (:314).  t of (ray i, sample s) is
 * tvals[i*t_ray_stride + s]; t_ray_stride = 0 shares one table (the deterministic coarse linspace). */
int32_t nerf_mlp_forward_rays(const float* rays_o, const float* rays_d, const float* tvals,
                              int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                              const void* packed, float* raw, int32_t precision, void* stream);

/* Density-only form of nerf_mlp_forward_rays: raw[..., 3] = sigma, bit for bit the value nerf_mlp_forward_rays writes there.
 * In a hierarchical render (N_importance > 0) the reference reads nothing else of the coarse network's output
 * (volume_renderer.py:335 `density_coarse = outputs[...,3]`; rgb and depth are composited from the fine outputs, :414-437), so
 * nerf_render_forward runs its coarse pass through this entry.  The network stops after the sigma head (feature_linear,
 * views_linears.0 and rgb_linear are not evaluated: 982 528 instead of 1 186 816 FLOP per point) and the rgb columns of `raw`
 * are written as 0, in every precision. */
int32_t nerf_mlp_forward_rays_density(const float* rays_o, const float* rays_d, const float* tvals,
                                      int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                      const void* packed, float* raw, int32_t precision, void* stream);

/* nerf_mlp_forward_rays for outputs that go to nerf_composite and nowhere else (the fine pass of nerf_render_forward): the
 * sigma column is bit for bit nerf_mlp_forward_rays'; the rgb columns are too, EXCEPT that they may be 0 for points whose
 * sigma is <= 0 -- compositing gives those samples alpha = 1 - exp(-relu(sigma) delta) = 0, hence weight 0, and multiplies their
 * colour by exactly zero (volume_renderer.py:67-96, :414-437), so rgb and depth out of nerf_composite are bit-identical either
 * way.  A 32-point tile (32 consecutive samples) without a single sigma > 0 skips the colour branch (17 % of its FLOP), in
 * every precision; how many tiles do is scene-dependent. */
int32_t nerf_mlp_forward_rays_for_compositing(const float* rays_o, const float* rays_d, const float* tvals,
                                              int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                              const void* packed, float* raw, int32_t precision, void* stream);

/* Dead k-step skipping (NERF_PREC_F32, the four inference entries above; exact): inside a 32-point tile, a step of a layer's
 * reduction whose two input features are zero at all 32 points -- a ReLU output that is off tile-wide -- would add
 * fma(w, +0, acc) = acc to every output, so the kernel does not issue its matrix instructions.  `raw` is bit-identical for
 * finite weights (a NaN / Inf weight times such a zero would have been NaN: a checkpoint that renders NaN anyway may do so in
 * fewer pixels).  How many steps are skipped is scene-dependent (17-30 % of them on the synthetic benchmark scene, close to
 * none with white-noise weights).  NERF_DEAD_KSTEP_SKIP=0 in the environment makes the kernel issue every instruction, for
 * A/B comparisons; the training entries below never skip.
 * Leading dead groups (same entries; exact): the steps are issued in groups of four, and where the groups a trunk layer's
 * reduction starts with are dead as a whole -- under a unit order (nerf_mi355x_order.h) the deadest steps come first -- the kernel
 * steps over that run without waiting for, or fetching, its weights, and fetches from the first group that runs.  A stepped-over
 * group adds nothing, exactly as its four skipped steps: `raw` is bit-identical.  Trunk layers 1-7 only: the views layer keeps the
 * per-step decisions alone (DESIGN.md section 2.1 says why).  NERF_DEAD_GROUP_SKIP=0 switches this path off
 * and leaves the per-step decisions as they are (its own A/B switch); NERF_DEAD_KSTEP_SKIP=0 switches off both. */

/* ---- training path (BASELINE config 3; fp32 only) ------------------------------------------------
 * Forward with activation save: as nerf_mlp_forward_rays, and additionally stores, row-major per
 * point (P = n_rays*n_samples; floats): pe [P,64] and dpe [P,32] (encodings in the reference's channel
 * order, zero padded), h0..h7 [P,256] each (post-ReLU, network.py:55-56), feature [P,256] (:62),
 * views [P,128] (post-ReLU, :66-67) -- in that order, nerf_train_save_floats(P) floats in total.
 * These are the tensors autograd would keep for network.py:49-74.  precision: NERF_PREC_F32 or NERF_PREC_F32X
 * (`packed` must be the stream of that precision); the backward kernels are fp32 either way. */
int64_t nerf_train_save_floats(int64_t n_points);
int32_t nerf_mlp_forward_rays_save(const float* rays_o, const float* rays_d, const float* tvals,
                                   int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                   const void* packed, float* raw, float* save, int32_t precision, void* stream);

/* Backward of the MLP (network.py:49-74 under autograd) for the points of nerf_mlp_forward_rays_save.
 * `packed_bwd` is the transposed weight stream of nerf_pack_model_bwd (nerf_packed_bwd_bytes(precision) bytes;
 * precision NERF_PREC_F32: exact fp32 MFMA chain, NERF_PREC_F32X: split-fp16 chain; weight gradients are fp32 MFMA);
 * `draw` [P,4] is d loss / d raw; `save` the forward's activation store; `gsave` scratch of
 * nerf_train_grad_floats(P) floats (receives every layer's pre-activation gradient).  Adds the 24
 * parameter gradients (state_dict order, nn.Linear layouts; the caller zeroes them) and, if `g_t` [P]
 * is given, writes d loss / d t through the points (x = o + d t, positional encoding included) -- the
 * path by which the coarse network is trained.
 * The ReLU masks come from the sign-bit blocks the SAVE forwards append behind the activation rows (nerf_train_save_floats
 * covers them; both precisions write the same layout, so a `save` of either forward is accepted as long as it was written by the
 * matching entry: full / for-compositing / density).  Both `save` and `gsave` regions hold their rows padded to a
 * multiple of 32 points (offsets are derived from the padded count, see csrc/nerf_mlp_f32.hip.inc TrainSave). */
int64_t nerf_train_grad_floats(int64_t n_points);
/* Dead-tile skipping (n_points a multiple of 32; exact): a tile of 32 consecutive points whose `draw` rows are
 * all zero has zero g_z rows, adds nothing to any parameter gradient and has zero g_t / g_x -- compositing writes such rows
 * wherever relu(sigma) = 0.  nerf_mlp_backward* drop those tiles from the chain launch and from every weight-gradient launch
 * (their rows in `gsave` are then left unwritten).  The number of live tiles of the call is left as an int32 at float offset
 * nerf_train_live_count_offset(n_points) of `gsave` (-1: the call ran without a list: ragged n_points, or
 * NERF_DEAD_TILE_SKIP=0 in the environment, which turns the skipping off for A/B comparisons). */
int64_t nerf_train_live_count_offset(int64_t n_points);
int64_t nerf_packed_bwd_bytes(int32_t precision);
int32_t nerf_pack_model_bwd(const float* const params[24], void* packed_bwd, int32_t precision, void* stream);
int32_t nerf_mlp_backward(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                          int64_t n_rays, int32_t n_samples, const void* packed_bwd, const float* draw,
                          const float* save, float* gsave, float* g_t, float* const grads[24], int32_t precision,
                          void* stream);

/* nerf_mlp_forward_rays_save for a fine pass whose `raw` goes to nerf_composite and whose `draw` will come from
 * nerf_composite_backward (training.RenderFunction): a 32-point tile without a single sigma > 0 stops after the sigma head
 * (rgb = 0 there, as nerf_mlp_forward_rays_for_compositing) and stores nothing past its h6 row (NERF_PREC_F32) / its h7 row
 * (NERF_PREC_F32X: no feature / views rows, no views bits).  CONTRACT: the `draw`
 * later given to nerf_mlp_backward with this `save` must be zero wherever sigma <= 0 -- nerf_composite_backward guarantees it --
 * so that the backward pass, which skips tiles with a zero incoming gradient, never reads those rows.  With
 * NERF_DEAD_TILE_SKIP=0 in the environment (or a point count that is not a multiple of 32) this is nerf_mlp_forward_rays_save. */
int32_t nerf_mlp_forward_rays_save_for_compositing(const float* rays_o, const float* rays_d, const float* tvals,
                                                   int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                                   const void* packed, float* raw, float* save, int32_t precision, void* stream);

/* Density-only twins for the COARSE pass of a training step.  In the reference's step only the coarse sigma is ever used
 * (it places the fine samples; the coarse colour is never composited, volume_renderer.py:385-397), so
 * d loss / d raw_coarse has identically zero rgb columns and the gradients of rgb_linear, views_linears.0 and
 * feature_linear of the coarse sub-model are exactly zero.  These entries skip that branch (both precisions): the forward
 * stops after the sigma head (raw = (0, 0, 0, sigma); feature / views rows are not stored), the backward starts at
 * g_h7 = w_alpha * g_sigma and leaves the three colour gradients as zeroed by the caller.  `draw`'s rgb columns are not
 * read.  `save` from the density forward must go to the density backward. */
int32_t nerf_mlp_forward_rays_save_density(const float* rays_o, const float* rays_d, const float* tvals,
                                           int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                                           const void* packed, float* raw, float* save, int32_t precision, void* stream);
int32_t nerf_mlp_backward_density(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                  int64_t n_rays, int32_t n_samples, const void* packed_bwd, const float* draw,
                                  const float* save, float* gsave, float* g_t, float* const grads[24], int32_t precision,
                                  void* stream);

/* Point-mode twins of the two calls above, for Network.forward itself under autograd (network.py:199-258: explicit
 * `inputs` [n_rays, n_samples, 3] and `viewdirs` [n_rays, 3] used AS GIVEN, no normalisation -- not o + d t):
 * nerf_mlp_forward_points_save = nerf_mlp_forward + the activation store; nerf_mlp_backward_points adds the 24
 * parameter gradients and, if `g_pts` [P,3] is given, writes d loss / d inputs (through the positional encoding).
 * d loss / d viewdirs comes from nerf_viewdirs_backward below (a separate, tiny launch: no caller of the reference needs it). */
int32_t nerf_mlp_forward_points_save(const float* pts, const float* viewdirs, int64_t n_rays, int32_t n_samples,
                                     const void* packed, float* raw, float* save, int32_t precision, void* stream);
int32_t nerf_mlp_backward_points(const float* pts, int64_t n_rays, int32_t n_samples, const void* packed_bwd,
                                 const float* draw, const float* save, float* gsave, float* g_pts,
                                 float* const grads[24], int32_t precision, void* stream);
/* d loss / d viewdirs [n_rays,3] of the Network.forward call whose backward just filled `gsave` (either chain): the ray's
 * direction reaches views_linears.0 through its 27-channel encoding, shared by the ray's samples.  `w_views` is the raw
 * views_linears.0.weight [128,283] (nn.Linear layout), `viewdirs` the forward's [n_rays,3]. */
int32_t nerf_viewdirs_backward(const float* gsave, int64_t n_rays, int32_t n_samples, const float* w_views,
                               const float* viewdirs, float* g_viewdirs, void* stream);

/* Gradients with respect to the rays (Renderer.render with rays_o / rays_d requiring grad; DESIGN section 2, "Gradients with
 * respect to the rays").  Three steps per training-style backward:
 *  1. nerf_mlp_backward_rays_x: nerf_mlp_backward (density_only == 0) / nerf_mlp_backward_density (density_only != 0) that, in
 *     addition, writes g_x [P,3] = d loss / d (o + d t) of every point when g_x is non-null (next to g_t, which stays optional;
 *     zero for the tiles that dead-tile skipping drops).  grads == NULL: the data-gradient chain alone -- no weight-gradient
 *     launch, nothing written to any gradient array (a frozen network).  g_t, g_x and the g_z rows in `gsave` are bit-identical
 *     to a call with grads, and to a call without g_x.
 *  2. nerf_rays_viewdirs_backward, right after the FINE pass's call 1 and before anything reuses its `gsave`: the fine pass's view
 *     direction v = d / |d| (rounded as the forward kernels round it) takes sum_s g_zv[ray, s] through views_linears.0's 27
 *     direction columns (`w_views`: the fine views_linears.0.weight [128,283]) and the normalisation:
 *     g_rays_d_view [n,3] = (g_v - v (v . g_v)) / |d|.  Reads the tile flags of `gsave`: dead tiles' unwritten rows are skipped.
 *  3. nerf_rays_backward: per ray, with the 64 coarse depths t_coarse (t_ray_stride 0: one shared table; 64: one row per ray),
 *     the coarse pass's g_x_coarse [n,64,3] (its incoming gradient is the sampler adjoint's), the merged depths t_sorted [n,192]
 *     and the fine pass's g_x_fine [n,192,3]:
 *       g_rays_o = sum_s g_x_coarse + sum_s g_x_fine,  g_rays_d = sum_s t_coarse g_x_coarse + sum_s t_sorted g_x_fine + g_rays_d_view.
 *     One wave per ray, fixed summation order (no atomics): deterministic.  g_x_coarse, g_x_fine, g_rays_d_view may be NULL
 *     (term left out).  f32 / f32x chains only, like nerf_mlp_backward. */
int32_t nerf_mlp_backward_rays_x(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                 int64_t n_rays, int32_t n_samples, const void* packed_bwd, const float* draw,
                                 const float* save, float* gsave, float* g_t, float* g_x, float* const grads[24],
                                 int32_t density_only, int32_t precision, void* stream);
int32_t nerf_rays_viewdirs_backward(const float* rays_d, int64_t n_rays, int32_t n_samples, const float* gsave,
                                    const float* w_views, float* g_rays_d_view, void* stream);
int32_t nerf_rays_backward(int64_t n_rays, const float* t_coarse, int64_t t_ray_stride, const float* g_x_coarse,
                           const float* t_sorted, const float* g_x_fine, const float* g_rays_d_view, float* g_rays_o,
                           float* g_rays_d, void* stream);

/* ---- masked (fast_sampling) fine pass of a training step ------------------------------------------------------------
 * The reference evaluates the fine network on the merged samples that survive ESS / ERT only (boolean indexing of
 * network.py:207-214, results scattered back into zeros :238-253, mask from volume_renderer.py:132-244, :359-369) and
 * autograd follows: masked samples give no parameter gradient and no gradient through their point.  Here the valid ids
 * are compacted on the device and the forward / backward work on the M compact rows; M never reaches the host.
 *
 * nerf_compact_valid: valid [n_points] (uint8, nerf_sample_fine's valid_sorted) -> index[0..M) = the ids with valid != 0 in
 * ASCENDING order, *count = M.  The fixed order makes the save layout, the live-tile lists and every sum repeatable
 * (nerf_render_forward's own compaction is atomic and unordered).  n_points <= 2^31 - 1 (NERF_ERR_INVALID_ARG beyond);
 * `workspace`: nerf_compact_valid_workspace_bytes(n_points) bytes. */
int64_t nerf_compact_valid_workspace_bytes(int64_t n_points);
int32_t nerf_compact_valid(const uint8_t* valid, int64_t n_points, int32_t* index, int32_t* count, void* workspace,
                           void* stream);
/* nerf_mlp_forward_rays_save_for_compositing on the listed points: `raw` rows are written at the point ids index[j] (the
 * caller zero-fills `raw`: a masked sample has raw = 0, network.py:238-253), the activation rows and the ReLU sign-bit
 * blocks at the COMPACT slot j, in the nerf_train_save_floats(n_rays * n_samples) layout.  Rows >= M are not
 * written, M need not be a multiple of 32 (the idle lanes of the last tile store duplicates behind row M - 1).  The
 * for-compositing rule applies per compact tile.  index / count as nerf_compact_valid leaves them (ids < n_rays * n_samples,
 * count <= n_rays * n_samples).  n_rays * n_samples <= 2^31 - 1 (NERF_ERR_INVALID_ARG beyond).  f32 / f32x. */
int32_t nerf_mlp_forward_rays_save_masked(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                          int64_t n_rays, int32_t n_samples, const int32_t* index, const int32_t* count,
                                          const void* packed, float* raw, float* save, int32_t precision, void* stream);
/* nerf_mlp_backward for a `save` of nerf_mlp_forward_rays_save_masked (same index / count).  `draw` [P,4] and g_t [P]
 * (nullable) are in the global layout, P = n_rays * n_samples: the rows of the listed points are gathered to compact rows
 * (rows >= M zero) together with the points o + d t, the chain and every weight-gradient kernel run in point mode over the
 * live compact tiles (tiles behind row M - 1 are never live; with NERF_DEAD_TILE_SKIP=0 every occupied tile is), and g_t of a
 * listed point = g_x . d is scattered back; g_t is 0 at unlisted ids.  `gsave`: nerf_train_grad_floats(P) floats (rows in the
 * compact layout), `workspace`: nerf_mlp_backward_masked_workspace_bytes(P) bytes.  P must be a multiple of 32
 * (NERF_ERR_UNSUPPORTED otherwise; n_samples = 192 always is) and <= 2^31 - 1 (NERF_ERR_INVALID_ARG). */
int64_t nerf_mlp_backward_masked_workspace_bytes(int64_t n_points);
int32_t nerf_mlp_backward_masked(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                                 int64_t n_rays, int32_t n_samples, const int32_t* index, const int32_t* count,
                                 const void* packed_bwd, const float* draw, const float* save, float* gsave, float* g_t,
                                 float* const grads[24], int32_t precision, void* workspace, void* stream);

/* Adjoint of nerf_composite (autograd of volume_renderer.py:414-432 with :67-96): g_rgb [n,3], g_depth [n]
 * (nullable) -> g_raw [n,S,4] and, if given, g_t [n,S] (the direct dependence of the image on the sample
 * depths through delta_k = t_{k+1}-t_k and the depth sum; the last sample's delta is the constant 1e10).  S <= 192.  The relu
 * mask (sigma > 0) and whether clamp(1 - alpha, 1e-10, 1) passes the gradient (1e-10 <= 1 - alpha <= 1) are decided in fp32 exactly
 * as nerf_composite computes them; everything else is evaluated in float64 from the inputs.  Rows of g_raw are exactly zero wherever
 * sigma <= 0 (relu: alpha = 0, weight 0) -- what the dead-tile skipping of nerf_mlp_backward* feeds on. */
int32_t nerf_composite_backward(const float* raw, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                                int32_t n_samples, int32_t white_bkgd, const float* g_rgb, const float* g_depth,
                                float* g_raw, float* g_t, void* stream);

/* Adjoint of nerf_sample_fine (autograd of volume_renderer.py:126-154, :247-264, :349-356): gradient of the
 * merged depths g_t_sorted [n,192] -> g_raw_coarse [n,64,4] (channel 3 only; the reference does NOT detach
 * the coarse weights, so the coarse network trains through the sample positions).  The bin of every fine sample, the
 * `denom < 1e-5` branch, its slot in t_sorted (ties: coarse first) and the relu / clamp-pass masks are the forward's own fp32
 * decisions; on them the adjoint is evaluated in float64 from the inputs.  The rgb channels of g_raw_coarse are written as 0, and
 * those of raw_coarse are not read. */
int32_t nerf_sample_fine_backward(const float* raw_coarse, const float* t_coarse, const float* u, int64_t n_rays,
                                  const float* t_sorted, const float* g_t_sorted, float* g_raw_coarse, void* stream);

/* Fused gradient clipping + Adam over up to 48 tensors in one launch.  Replaces
 * clip_grad_value_(parameters, 40) (src/train/trainers/trainer.py:59) followed by torch.optim.Adam.step()
 * as configured in src/train/optimizer.py:21-24 (betas (0.9, 0.999), no amsgrad; weight decay added to the
 * gradient).  The pointer arrays are HOST arrays of DEVICE pointers; `step` is the 1-based step count;
 * clip_value <= 0 disables clipping.  The six hyper-parameters are doubles (Python floats): the fp32 constants of
 * the update are formed in double on the host, as torch forms them, and rounded once:
 *     w1 = (float)(1 - beta1), b2 = (float)beta2, w2 = (float)(1 - beta2), bc2s = (float)sqrt(1 - beta2^step),
 *     s = (float)-(lr / (1 - beta1^step)), and eps, weight_decay, clip_value each rounded to fp32.
 * Per element, every operation correctly rounded fp32 on its own, denormals kept:
 *     g = clamp(g, -clip, clip) (a NaN gradient stays NaN, as clamp_; +-inf becomes +-clip);  g = g + wd * p (wd != 0);
 *     m = m + (g - m) * w1 if w1 < 0.5, else g - (g - m) * (1 - w1)  (the two forms of torch's lerp: beta1 <= 0.5 takes the second);
 *     v = v * b2 + (g * g) * w2;  denom = sqrt(v) / bc2s + eps;  p = p + s * (m / denom).
 * A tensor with numel[i] == 0 is stepped over and its four pointers are not examined (an empty device tensor has a null data
 * pointer); numel[i] < 0, n_tensors outside 1..48 and step <= 0 are NERF_ERR_INVALID_ARG ("bad size"), a null pointer of a tensor
 * with elements is NERF_ERR_INVALID_ARG ("null tensor"); nothing is launched then.  grads are read only. */
int32_t nerf_adam_step(int32_t n_tensors, float* const params[], const float* const grads[], float* const exp_avg[],
                       float* const exp_avg_sq[], const int64_t numel[], double lr, double beta1, double beta2, double eps,
                       double weight_decay, double clip_value, int64_t step, void* stream);

/* Weight / bias gradient of one nn.Linear (or a column block of it): for o < n_out, i < n_in
 *     dw[o*ldw + wc0 + i] += sum_p dz[p*ldz + zc0 + o] * hin[p*ldh + hc0 + i],   db[o] += sum_p dz[p*ldz + zc0 + o]
 * i.e. autograd's grad_weight = grad_out^T @ input, grad_bias = grad_out.sum(0) for network.py:22-47;
 * `dw` (and `db`, optional) accumulate with float atomics and must be zeroed by the caller; dw is in the
 * nn.Linear [out, in] layout (ldw = in_features), so concatenated inputs (skip, view) are two calls with
 * different wc0.  n_out, n_in <= 256. */
int32_t nerf_wgrad(const float* dz, int64_t ldz, int32_t zc0, int32_t n_out, const float* hin, int64_t ldh,
                   int32_t hc0, int32_t n_in, float* dw, int64_t ldw, int32_t wc0, float* db, int64_t n_points,
                   void* stream);

/* Hierarchical sampling + merge.  raw_coarse [n,64,4] (sigma = channel 3, pre-ReLU), t_coarse [64],
 * u [128] -> t_sorted [n,192] (ascending union of coarse and fine depths), optional t_fine [n,128].
 * Replaces ReLU of the coarse density (volume_renderer.py:335-338), weights_computation (:67-96),
 * fine_sample_points' deterministic branch (:126-154, :247-264) incl. its index clamp to 61, and the
 * cat + torch.sort of depths (:349-353); the sorted POINTS (:354-356) are regenerated as o + d*t.
 * If `valid_sorted` [n,192] (uint8) is non-NULL the fast_sampling branch is evaluated too: ESS (coarse
 * weight < weights_threshold around the sample, strict for rays with max sigma > 0.5) and ERT (coarse
 * transmittance < ert_threshold) masks and the empty-ray test (:116-123, :132-133, :158-193), merged
 * through the sort with the always-valid coarse samples (:359-369).
 * Rules of the merge: t_coarse and u are ascending, and with valid_sorted every depth is > 0 (the validity of a fine sample rides
 * through the merge as the sign of its depth: a depth of 0 would come out invalid).  Where a fine depth equals a coarse depth the
 * coarse sample comes first, in t_sorted's order and therefore in valid_sorted's; equal fine depths keep the order of their u. */
int32_t nerf_sample_fine(const float* raw_coarse, const float* t_coarse, const float* u,
                         int64_t n_rays, float* t_sorted, float* t_fine, uint8_t* valid_sorted,
                         float weights_threshold, float ert_threshold, void* stream);

/* Final activations + alpha compositing.  raw [n,S,4], t per (ray,sample) as above ->
 * rgb [n,3], depth [n], optional weights [n,S].  Replaces volume_renderer.py:414-432:
 * sigmoid(rgb), relu(sigma), weights_computation, the two sums and the white background. */
int32_t nerf_composite(const float* raw, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                       int32_t n_samples, int32_t white_bkgd, float* rgb, float* depth,
                       float* weights, void* stream);

/* Pinhole ray generation on the device.  Replaces src/datasets/nerf/blender.py:102-127
 * (float64 math, float32 result, unit directions): pixel id -> u = id % W, v = id / W,
 * dirs = [(u-W/2)/f, -(v-H/2)/f, -1], rays_d = normalize(R dirs), rays_o = t.  `c2w` is a HOST array,
 * row-major 3x4.  Pixels are pixel_begin .. pixel_begin+n_pixels-1 (row-major image order, a rank's
 * tile) or, if `pixel_ids` (DEVICE int64 [n_pixels]) is given, that list (a training batch). */
int32_t nerf_generate_rays(const double c2w[12], int32_t H, int32_t W, double focal, int64_t pixel_begin,
                           int64_t n_pixels, const int64_t* pixel_ids, float* rays_o, float* rays_d, void* stream);

/* Evaluator sums, src/evaluators/nerf.py: sums2[0] = sum over all values of
 * (clip(pred,0,1) - clip(gt,0,1))^2 (:96-100), sums2[1] = sum of the evaluator's psnr_metric
 * integrand (:23-30) whose uint8 subtraction and squaring wrap mod 256.  `sums2` is a
 * DEVICE double[2], zeroed by the call; mean = sum / n_values, PSNR = 10 log10(peak^2 / mean). */
int32_t nerf_image_metrics(const float* pred, const float* gt, int64_t n_values, double* sums2, void* stream);

/* SSIM sum of src/evaluators/nerf.py:49-77: skimage.metrics.structural_similarity on the uint8 images
 * (win_size 7, channel_axis 2: uniform 7x7 window, sample covariance, K1 .01, K2 .03, data_range 255).
 * pred, gt: [H,W,3] float in [0,1] (clipped and truncated to uint8 as the evaluator does); *sum1 (DEVICE
 * double, zeroed by the call) = sum of the SSIM map over the (H-6)x(W-6) interior and 3 channels;
 * SSIM = sum / ((H-6)(W-6)3).  skimage is not vendored/pinned by the reference (requirements.txt): the
 * published algorithm is restated. */
int32_t nerf_image_ssim(const float* pred, const float* gt, int32_t H, int32_t W, double* sum1, void* stream);

/* Bytes of scratch nerf_render_forward needs for n_rays rays. */
int64_t nerf_render_workspace_bytes(int64_t n_rays, int32_t n_importance, int32_t fast_sampling);

/* Renderer.render for already-flattened rays [n,3]: coarse pass, hierarchical sampling, fine pass,
 * compositing (volume_renderer.py:306-432).  n_importance is 0 (coarse only) or 128.  t_coarse [64]
 * and u [128] are the host-built torch.linspace tables (bit-sensitive).
 * fast_sampling != 0 selects the ESS/ERT masked fine pass (off in every reference config):
 * only merged samples that survive the masks go through the fine network (device-side compaction),
 * the rest contribute raw = 0 exactly as network.py:238-253 does.  Outputs rgb [n,3], depth [n]. */
int32_t nerf_render_forward(const float* rays_o, const float* rays_d, int64_t n_rays,
                            const void* packed_coarse, const void* packed_fine,
                            const float* t_coarse, const float* u, int32_t n_importance,
                            int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                            float weights_threshold, void* workspace,
                            int64_t workspace_bytes, float* rgb, float* depth, void* stream);

/* ---- stochastic sampling (the reference's task == "train" mode) -----------------------------------------------------
 * Coarse jitter of volume_renderer.py:48-60: t_coarse [n,64] = lower + (upper - lower) * jitter [n,64], with mids =
 * 0.5 (t[1:] + t[:-1]), lower = [t0, mids], upper = [mids, t63] of the host-built table t_linear [64]; every operation
 * separately rounded, bit-equal to the CPU torch expression. */
int32_t nerf_stratified_samples(const float* t_linear, const float* jitter, int64_t n_rays, float* t_coarse, void* stream);

/* nerf_sample_fine with per-ray tables: the coarse depths of ray r are t_coarse[r * t_ray_stride + s] (stride 0 or 64) and
 * its u are u[r * u_ray_stride + k] (stride 0 or 128, any order: random u of volume_renderer.py:143-147).  t_sorted =
 * torch.sort(cat(t_coarse, t_fine)) of the reference's arithmetic (torch_sum62 order, index clamp to 61); the kernel sorts
 * each ray's u first (t_sorted depends only on the multiset of fine depths).  t_fine, if given, comes back in the caller's u
 * order.  Both strides 0: exactly nerf_sample_fine.  valid_sorted (fast_sampling) with a non-zero stride: NERF_ERR_INVALID_ARG. */
int32_t nerf_sample_fine_rays(const float* raw_coarse, const float* t_coarse, int64_t t_ray_stride, const float* u,
                              int64_t u_ray_stride, int64_t n_rays, float* t_sorted, float* t_fine, uint8_t* valid_sorted,
                              float weights_threshold, float ert_threshold, void* stream);

/* Adjoint of nerf_sample_fine_rays (same strides; both 0: exactly nerf_sample_fine_backward), float64 accumulation.  The
 * jittered coarse depths get no gradient: in the reference they depend on no parameter. */
int32_t nerf_sample_fine_rays_backward(const float* raw_coarse, const float* t_coarse, int64_t t_ray_stride, const float* u,
                                       int64_t u_ray_stride, int64_t n_rays, const float* t_sorted, const float* g_t_sorted,
                                       float* g_raw_coarse, void* stream);

/* Bytes of scratch nerf_render_forward_stochastic needs for n_rays rays. */
int64_t nerf_render_stochastic_workspace_bytes(int64_t n_rays, int32_t n_importance);

/* nerf_render_forward in the reference's training sampling mode.  jitter [n,64] (nullable: the shared t_coarse table) and
 * u_rays [n,128] (nullable: the shared u table) are the reference's two torch.rand draws, in its order.  The output does not
 * depend on the 2^20-ray blocking.  n_importance 0 or 128; precision NERF_PREC_F32 or NERF_PREC_F32X (fp16 and fast_sampling:
 * NERF_ERR_INVALID_ARG).  With both draws NULL this computes exactly what nerf_render_forward does. */
int32_t nerf_render_forward_stochastic(const float* rays_o, const float* rays_d, int64_t n_rays,
                                       const void* packed_coarse, const void* packed_fine,
                                       const float* t_coarse, const float* u, const float* jitter, const float* u_rays,
                                       int32_t n_importance, int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                                       float weights_threshold, void* workspace, int64_t workspace_bytes,
                                       float* rgb, float* depth, void* stream);

/* ---- iso-surface of a scalar grid (the reference's src/utils/mesh_utils.py:8-46, extract_mesh: density on a grid, then a
 * triangle mesh of {f = level}; DESIGN section 2.8 lists where this departs from that function) -------------------------------
 * The value of grid point (i, j, k) is field[((i*ny + j)*nz + k) * stride]: stride 1 for a dense [nx,ny,nz] grid, 4 to read
 * sigma out of a `raw` [P,4] buffer (pass raw + 3).  Marching tetrahedra over the six-tetrahedra (Kuhn) split of every cell:
 * tetrahedron q of cell c is {c, c + e_a, c + e_a + e_b, c + (1,1,1)} for the q-th permutation (a, b, c) of the axes in
 * lexicographic order.  A point is inside iff f > level (NaN is not); an edge (p, p + e), e in {0,1}^3 \ 0, carries a vertex
 * iff its endpoints differ, at x_p + tau (x_{p+e} - x_p) per axis with tau = (level - f_p) / (f_{p+e} - f_p) and
 * x = fp32(origin + idx * step) (that in float64, rounded once); every other operation is separately rounded fp32.  Vertex ids
 * ascend with (owner id p, edge type 4 e_x + 2 e_y + e_z), triangles with (cell id, tetrahedron, triangle); (v1 - v0) x (v2 - v0)
 * points from inside to outside.  The mesh is indexed (one vertex per crossed edge), closed and consistently oriented wherever
 * the level set stays off the grid boundary, and open where the boundary cuts it.  No atomics: two runs write the same bytes.
 *
 * Two phases, because the sizes depend on the data: nerf_isosurface_count fills `workspace`
 * (nerf_isosurface_workspace_bytes: 4 bytes per point + 8 per 256 points) and writes counts[0] = V, counts[1] = T; the
 * caller reads them, allocates vertices [V,3] and triangles [T,3] (or more rows: the rest is left untouched) and calls
 * nerf_isosurface_emit with the same field, sizes, level and workspace.  Emit takes the topology from the workspace alone, so it
 * writes inside those rows whatever the field holds by then.  A grid of more than 2^31 - 1 points is refused
 * (NERF_ERR_INVALID_ARG; workspace_bytes returns -1); V or T beyond int32 cannot be known when the call is enqueued: counts is
 * then (-1, -1) and emit must not follow.  Any dimension of 0 or 1 means no cells: success, counts = (0, 0), emit is a no-op.
 * origin[3] and step[3] are HOST arrays. */
int64_t nerf_isosurface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int32_t nerf_isosurface_count(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level,
                              void* workspace, int32_t* counts, void* stream);
int32_t nerf_isosurface_emit(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level,
                             const double origin[3], const double step[3], const void* workspace,
                             float* vertices, int32_t* triangles, void* stream);

/* ---- occupancy grid: skip the samples of a render that lie in empty space ------------------------------
 * Grid: nx x ny x nz points (every size >= 2, at most 2^31 - 1 points), values laid out as for nerf_isosurface_* (stride 1, or 4
 * for the sigma column of a `raw` buffer).  Cell (i, j, k) lies between the points i..i+1, j..j+1, k..k+1; its id is
 * (i*(ny-1) + j)*(nz-1) + k.  A cell is OCCUPIED iff some grid point in [i-r, i+1+r] x [j-r, j+1+r] x [k-r, k+1+r] (clipped to the
 * grid, r = dilate >= 0) has f > level or is NaN (NaN counts as occupied, the conservative side; nerf_isosurface_*'s "inside"
 * goes the other way).  Bitfield: bit (id & 31) of the 32-bit word (id >> 5); nerf_occupancy_words gives the number of words,
 * rounded up to an even number (-1 for a refused size); the unused tail bits are 0.  No atomics: two builds write the same bytes.
 *
 * Lookup of a sample (ray r, depth t): x = fadd(o, fmul(d, t)) -- the forward kernels' two roundings -- and per axis
 * c = floorf(fmul(fsub(x, box_min), inv_step)), with box_min = fp32(min) and inv_step = fp32((n - 1) / (max - min)) computed in
 * float64 by the caller and rounded once.  The sample is KEPT if any c is outside [0, n-2] (outside the box counts as occupied),
 * if anything is NaN, or if the cell's bit is set.  nerf_occupancy_mark writes
 *     valid[r, s] = (and_with_existing ? valid[r, s] != 0 : 1) & keep(sample)
 * for t = tvals[r * t_ray_stride + s] (stride 0: one shared table); n_rays * n_samples <= 2^31 - 1.  dims, box_min and inv_step
 * are HOST arrays. */
int64_t nerf_occupancy_words(int32_t nx, int32_t ny, int32_t nz);
int32_t nerf_occupancy_build(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level,
                             int32_t dilate, uint32_t* bits, void* stream);
int32_t nerf_occupancy_mark(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride,
                            int64_t n_rays, int32_t n_samples, const uint32_t* bits, const int32_t dims[3],
                            const float box_min[3], const float inv_step[3], int32_t and_with_existing, uint8_t* valid,
                            void* stream);

/* The grid's memory across refreshes (training with a grid): near sigma = 0 the sign of a grid point flickers
 * from one evaluation to the next, so every point carries an age, the number of refreshes since it was last above the level:
 *     hit(p) = field[p*stride] > level || isnan(field[p*stride])
 *     age[p] = hit ? 0 : (age[p] == 255 ? 255 : age[p] + 1)
 *     on[p]  = age[p] < hold ? 1.0f : -1.0f                      (dense, stride 1)
 * build(on, 1, nx, ny, nz, 0.0f, dilate, bits) then gives the bitfield of the points hit within the last `hold` refreshes: with hold
 * = 1 the bytes of a direct build from the field, with hold = 2 (dilation being a union over points) the bytewise OR of the last two
 * direct builds.  The caller fills `age` (one byte per point) with 255 before the first call.  hold in [1, 255]; 0 <= n_points <=
 * 2^31 - 1, n_points == 0 is a no-op; `on` may be `field` itself when stride == 1.  Size and range checks come before any pointer is
 * looked at (NERF_ERR_INVALID_ARG), as for nerf_occupancy_build.  One thread per point, no atomics. */
int32_t nerf_occupancy_age(const float* field, int64_t stride, int64_t n_points, float level, int32_t hold,
                           uint8_t* age, float* on, void* stream);

/* nerf_render_forward with occupancy culling.  occ_coarse / occ_fine (each nullable) are the bitfields looked up for the 64
 * coarse depths / the 192 merged depths (normally built from the coarse / the fine model's density; occ_fine is ignored when
 * n_importance is 0).  A pass with a bitfield evaluates the kept samples only (device-side compaction, as fast_sampling does) and
 * leaves raw = 0 at the others; nerf_sample_fine and nerf_composite both apply relu(sigma), so rgb and depth are bit-equal to
 * nerf_render_forward's wherever every culled sample has a true sigma <= 0.  With fast_sampling the fine list is the sampler's
 * mask AND the lookup.  With both bitfields NULL it launches what nerf_render_forward launches (dims, box_min, inv_step are then
 * not read).  `evaluated`: nullable DEVICE int64[2], zeroed by the call, receives the numbers of coarse and of fine points
 * evaluated, summed over the ray blocks (one single-thread launch per pass and block).  NERF_PREC_F32 / NERF_PREC_F32X only
 * (NERF_ERR_UNSUPPORTED otherwise: the fp16 far-plane guard is not defined on a culled list); n_rays * 192 <= 2^31 - 1
 * (NERF_ERR_INVALID_ARG).  workspace: nerf_render_occupancy_workspace_bytes (nerf_render_workspace_bytes with the fine mask and
 * list whatever fast_sampling is, plus the coarse mask [n,64] and its list). */
int64_t nerf_render_occupancy_workspace_bytes(int64_t n_rays, int32_t n_importance, int32_t fast_sampling);
int32_t nerf_render_forward_occupancy(const float* rays_o, const float* rays_d, int64_t n_rays,
                                      const void* packed_coarse, const void* packed_fine,
                                      const float* t_coarse, const float* u, int32_t n_importance,
                                      int32_t white_bkgd, int32_t precision, int32_t fast_sampling,
                                      float weights_threshold, const uint32_t* occ_coarse, const uint32_t* occ_fine,
                                      const int32_t dims[3], const float box_min[3], const float inv_step[3],
                                      int64_t* evaluated, void* workspace, int64_t workspace_bytes,
                                      float* rgb, float* depth, void* stream);

/* ---- geometry outputs: density gradient, surface normal and opacity ---------------------------------------
 * Definitions.  For sample i of a ray, with raw sigma_i the pre-activation density of the network that is composited (the fine one;
 * the coarse one when n_importance == 0) at x_i = fadd(o, fmul(d, t_i)):
 *     g_i = grad_x raw sigma(x_i): the data-gradient chain's g_x for an incoming gradient of 1 on sigma and 0 on rgb -- back through
 *           alpha_linear, the eight trunk layers with the skip, and the positional encoding's derivative; no view branch;
 *     n_i = -g_i / |g_i| if raw sigma_i > 0 and g_i . g_i > 0, else the zero vector; separately rounded fp32:
 *           gg = fadd(fadd(fmul(gx, gx), fmul(gy, gy)), fmul(gz, gz)), r = sqrt(gg), n = -g / r, square root and division both
 *           correctly rounded (the instruction sequences are written down in csrc/nerf_normals.hip.inc), no reciprocal shortcut;
 *     w_i = nerf_composite's weights (volume_renderer.py:67-96), from the same device function: bit-equal to its `weights` output;
 *     acc = sum_i w_i,  normal = sum_i w_i n_i, both summed left to right over the samples as nerf_composite sums (acc is the sum
 *           nerf_composite subtracts from 1 for the white background).  The normal is NOT renormalised: |normal| <= acc; callers
 *           normalise for display.
 *
 * nerf_density_gradient: sigma [P] (nullable) = raw sigma and grad [P,3] = g at the P = n_rays * n_samples points o + d t (t of
 * (ray i, sample s) at tvals[i*t_ray_stride + s], stride 0: one shared table).  With n_samples = 1 and t = 0 this is a plain point
 * list: fadd(o, fmul(d, 0)) = o for finite d.  sigma is bit for bit column 3 of nerf_mlp_forward_rays_density.
 * positive_only != 0: grad is exactly zero wherever raw sigma <= 0, and 32-point tiles without any density are dropped from the chain
 * (dead-tile skipping, above); elsewhere the values are those of positive_only == 0.
 * The points are cut into blocks of whole rays; per block: nerf_mlp_forward_rays_save_density, one small kernel that turns raw into
 * the chain's incoming gradient (0, 0, 0, seed) and copies sigma out, and nerf_mlp_backward_rays_x(density_only = 1, grads = NULL) --
 * all ordered on `stream`, no host sync.  The result does not depend on the blocking.  `workspace` holds one block: its TrainSave,
 * TrainGrad, raw and incoming gradient.  A block of r rays fits if
 *     workspace_bytes >= nerf_density_gradient_point_bytes() * r * n_samples      (r * n_samples rounded up to a multiple of 32),
 * and the entry takes the largest r <= floor(workspace_bytes / point_bytes / n_samples) whose layout fits: the caller bounds the
 * memory, not the frame.  NERF_ERR_WORKSPACE if that is no ray at all.  n_samples <= 192 (NERF_ERR_INVALID_ARG).  `packed` /
 * `packed_bwd`: nerf_pack_model / nerf_pack_model_bwd of `precision`; NERF_PREC_F32 and NERF_PREC_F32X only (NERF_ERR_UNSUPPORTED). */
int64_t nerf_density_gradient_point_bytes(void);
int32_t nerf_density_gradient(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                              int32_t n_samples, const void* packed, const void* packed_bwd, int32_t positive_only, float* sigma,
                              float* grad, int32_t precision, void* workspace, int64_t workspace_bytes, void* stream);

/* raw [n,S,4], t as for nerf_composite, grad [n,S,3] (g of the definitions) -> normal [n,3], acc [n].  S <= 192
 * (NERF_ERR_INVALID_ARG).  One wave per ray; lane l prepares samples l, l + 64, l + 128, then every lane walks the samples in order
 * (csrc/nerf_normals.hip.inc): no reduction tree, no atomics, two runs write the same bytes.  rgb is not read, white_bkgd plays no
 * part.  grad rows of samples with raw sigma <= 0 are read but never used (they may hold anything, NaN included). */
int32_t nerf_composite_normals(const float* raw, const float* tvals, int64_t t_ray_stride, int64_t n_rays, int32_t n_samples,
                               const float* grad, float* normal, float* acc, void* stream);

/* ---- mesh clean-up: connected components of an indexed triangle mesh, and the filter that keeps whole components (DESIGN section
 * 2.11; what users of the reference's src/utils/mesh_utils.py:45 get from trimesh's split) ---------------------------------------
 * faces [T,3] int32 over the vertex ids 0..V-1.  Two vertices are connected when a face names both; components are the transitive
 * closure.  vertex_label[v] = the SMALLEST vertex id of v's component; a vertex that no face names is a component of its own with 0
 * faces.  face_label[t] = vertex_label of the face's first vertex.  A face with any index outside [0, V) joins nothing, has the label
 * -1, belongs to no component and is never read through (a guard against writing outside the buffers, not an error).  Duplicate and
 * degenerate faces (v0 == v1) are faces like any other.
 * Table: one row per component, ascending label: comp_label[c], comp_faces[c] (faces with that label), comp_vertices[c]; the caller
 * gives room for V rows (every vertex may be alone), the first C = *n_components (DEVICE int) are written, the rest is left untouched.
 * Lock-free union-find that always links the larger root under the smaller one: the root of a tree is its minimum whatever the
 * arrival order, the counts are integer atomic adds and the table is ordered by a scan, so two runs write the same bytes.
 * V = 0: C = 0 and every face label is -1.  T = 0: every vertex is its own component.  V or T above 2^31 - 1: NERF_ERR_INVALID_ARG
 * before any launch or pointer is looked at (workspace_bytes returns -1).  workspace: nerf_mesh_components_workspace_bytes(V, T),
 * which covers both nerf_mesh_components and nerf_mesh_filter_* (they use it one after the other).
 *
 * Filter: component `l` is kept iff keep[l] != 0 (keep: V bytes, indexed by LABEL, i.e. by the component's smallest vertex id).  The
 * kept vertices and faces come out in their original order, the faces re-indexed; vertex_index[i] is the old id of new vertex i (to
 * gather normals, colours, ...).  Faces with label -1 are dropped.  Two phases as for nerf_isosurface_*: nerf_mesh_filter_count
 * fills `workspace` and writes counts[0] = V', counts[1] = T'; the caller reads them, allocates out_vertices [V',3], out_faces [T',3]
 * and vertex_index [V'] (or more rows: the rest is left untouched) and calls nerf_mesh_filter_emit with the same sizes and
 * workspace.  Emit takes where it writes from the workspace alone.  No atomics. */
int64_t nerf_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int32_t nerf_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, void* workspace,
                             int32_t* vertex_label, int32_t* face_label, int32_t* comp_label, int32_t* comp_faces,
                             int32_t* comp_vertices, int32_t* n_components, void* stream);
int32_t nerf_mesh_filter_count(const int32_t* vertex_label, const int32_t* face_label, const uint8_t* keep,
                               int64_t n_vertices, int64_t n_faces, void* workspace, int32_t* counts, void* stream);
int32_t nerf_mesh_filter_emit(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces,
                              const void* workspace, float* out_vertices, int32_t* out_faces, int32_t* vertex_index,
                              void* stream);

/* ---- multiresolution hash-grid encoding (instant-NGP; the reference's src/models/encoding/hashencoder) -------
 * x [B,D] in [0,1], emb [offsets[L],C], out / grad_out [B,L*C] (level-major columns: level l owns columns l*C .. l*C+C-1), fp32.
 * D in {2,3,4}, C in {1,2,4,8}, 1 <= L <= 32.  Level l is the rows offsets[l] .. offsets[l+1]-1 of emb; n = their number.
 * offsets_host (int32 [L+1], increasing, offsets[0] >= 0) and scales_host (float [L]) are HOST arrays; they travel inside the kernel
 * arguments: no device allocation, no workspace, no host sync.  scales_host[l] is the level's grid scale, which the caller computes
 * (nerf_replication_amd/hashgrid.py: float32(exp2(l * log2(per_level_scale)) * base_resolution - 1), in double, rounded once).
 * Per point and level, in fp32 with every multiply and add rounded on its own:
 *     pos_d = x_d * scale + 0.5,  g_d = floor(pos_d),  f_d = pos_d - g_d,  resolution = uint32(ceil(scale)) + 1
 *     corner idx in 0 .. 2^D-1 sits at g_d + bit_d(idx) and weighs w = 1 * prod_d (bit_d(idx) ? f_d : 1 - f_d), d ascending
 *     row(corner), in uint32 with wrap-around: stride = 1, index = 0; for d = 0..D-1 while stride <= n: index += g_d * stride,
 *         stride *= resolution + 1; if then stride > n: index = XOR_d g_d * prime_d (1, 19349663, 83492791, 25165843); row = index mod n
 *     out[b, l*C + c] = sum over idx ascending, from 0, of w * emb[offsets[l] + row, c]
 * Every row is reduced modulo n, so inputs outside [0,1], infinities and NaN give unspecified values but never an access outside the
 * level.
 * nerf_hashgrid_backward: grad_emb (may be NULL) [offsets[L],C] is ACCUMULATED into with no-return fp32 atomic adds,
 *     grad_emb[offsets[l] + row, c] += w * grad_out[b, l*C + c]  (the caller zeroes it; the arrival order, hence the last bits, vary
 *     from run to run); grad_x (may be NULL) [B,D] is WRITTEN: the derivative of the forward with respect to x inside the cell,
 *     sum_l sum_c grad_out[b, l*C + c] * sum over the corners of the other axes of scale * prod_(a != d) (their factor) * (emb[right,
 *     c] - emb[left, c]), recomputed from x and emb (nothing is kept from the forward).  emb is read only when grad_x is given.
 * emb, out and grad_out must be aligned to 4*C bytes (rows are moved as vectors).
 * Refused before any launch, with nerf_last_error set: D, C or L outside the lists above (NERF_ERR_UNSUPPORTED); B <= 0 (unlike the
 * ray entries, an empty batch is not a no-op here), B*L*C or B*D above 2^31 - 1 (the kernels index with 32 bits: encode in chunks),
 * offsets that do not increase, null or misaligned pointers (NERF_ERR_INVALID_ARG). */
int32_t nerf_hashgrid_forward(const float* x, const float* emb, int64_t B, int32_t D, int32_t C, int32_t L,
                              const int32_t offsets_host[], const float scales_host[], float* out, void* stream);
int32_t nerf_hashgrid_backward(const float* x, const float* emb, const float* grad_out, int64_t B, int32_t D, int32_t C, int32_t L,
                               const int32_t offsets_host[], const float scales_host[], float* grad_emb, float* grad_x,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_H */
