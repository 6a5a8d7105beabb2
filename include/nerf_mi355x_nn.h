/* nerf_mi355x_nn.h -- small-network entries of libnerf_mi355x.so: a fused ReLU MLP on fp32 MFMA, and the ray-side glue of a hash-grid
 * radiance field built on it (MI355X, gfx950).
 *
 * A second header of the same library: nerf_mi355x.h keeps the rendering surface, this one the networks that sit behind an
 * encoding (the reference's src/models/img_fit/network.py:24-38, a density or colour head).  Conventions, nerf_status and
 * nerf_last_error() are those of nerf_mi355x.h: every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated
 * otherwise; inputs are borrowed, outputs are caller-allocated; `stream` is a hipStream_t (NULL = default stream); calls only enqueue
 * work: no device allocation, no library-owned memory, no host synchronisation, safe under stream capture; the return value is 0 or a
 * negative nerf_status, and nerf_last_error() gives the message of the calling thread's last failure.
 */
#ifndef NERF_MI355X_NN_H
#define NERF_MI355X_NN_H

#include "nerf_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header's contracts; nerf_abi_version() (the core header) does not move when it does. */
#define NERF_NN_ABI_VERSION 1
int32_t nerf_nn_abi_version(void);

enum nerf_nn_activation {
  NERF_NN_ACT_NONE = 0,        /* y = z */
  NERF_NN_ACT_SIGMOID = 1      /* y = 1 / (1 + expf(-z)), correctly rounded division */
};

/* ---- fused MLP ------------------------------------------------------------------------------------------------
 *     h_0 = relu(W_0 x + b_0),   h_i = relu(W_i h_{i-1} + b_i)  for 0 < i < n_hidden,   z = W_out h_last + b_out,   y = act(z)
 * x [B,in_dim], out [B,out_dim].  The layers are nn.Linear tensors as they stand: W_0 [width,in_dim], W_i [width,width],
 * W_out [out_dim,width], row-major [out,in]; b_i [width], b_out [out_dim].
 * `weights` and `biases` are HOST arrays of n_hidden + 1 device pointers -- the hidden layers in order, then the output layer.  The
 * pointers travel inside the kernel arguments and the kernels read the tensors themselves: there is no packed copy, so a call sees
 * the values the tensors hold when its kernel runs in stream order (an in-place optimizer step between two calls is seen by the
 * second).
 * Domain: 1 <= in_dim <= 256, width in {64, 128}, 1 <= n_hidden <= 8, 1 <= out_dim <= 16, activation a nerf_nn_activation,
 * 1 <= B <= 8 388 607 (B * 256 stays below 2^31; run larger batches in chunks).
 *
 * Arithmetic: fp32.  Every layer is a chain of v_mfma_f32_32x32x2_f32 whose accumulator starts at the bias and takes the products of
 * one point in ascending order of the input feature, two features per MFMA; ReLU is fmaxf(., 0).  The result of a point depends on
 * that point's row alone -- not on B, on its position in the batch or on `save`.
 *
 * nerf_fused_mlp_forward: writes out.  save == NULL: inference.  Otherwise save receives, with the same instruction sequence (out is
 * bit-identical), the post-ReLU rows of every hidden layer: n_hidden blocks, block i = h_i as [B,width] row-major, one behind the
 * other with no padding inside or between them: nerf_fused_mlp_save_floats(B, width, n_hidden) = n_hidden * B * width floats.
 *
 * nerf_fused_mlp_backward: given x, the forward's out (read only with NERF_NN_ACT_SIGMOID; may be NULL otherwise) and save, and
 * grad_out [B,out_dim], ONE kernel computes
 *     dz_out = grad_out                         (none)      or   (grad_out * y) * (1 - y)      (sigmoid, y = out)
 *     dz_i   = (W_{i+1}^T dz_{i+1}) * (h_i > 0)  for i = n_hidden - 1 .. 0   (W_{n_hidden} = W_out; exactly 0 where h_i is 0)
 *     grad_x = W_0^T dz_0                        only if grad_x != NULL, [B,in_dim]
 * and WRITES them (no atomics, bit-reproducible from run to run): gsave holds n_hidden blocks [B,width], block i = dz_i, and behind
 * them one block [B,out_dim] = dz_out: nerf_fused_mlp_grad_floats(B, width, n_hidden, out_dim) = n_hidden * B * width + B * out_dim
 * floats, no padding.  Then the entry enqueues, for every layer i whose grad_weights[i] is not NULL, one weight-gradient launch (the
 * code behind nerf_wgrad), and one launch for the bias gradients of all layers (float64 partial sums over 1024 rows each, rounded
 * once):
 *     grad_weights[i][o,k] += sum_p dz_i[p,o] * in_i[p,k]     (in_0 = x, in_i = h_{i-1}),      grad_biases[i][o] += sum_p dz_i[p,o]
 * These ACCUMULATE with fp32 atomic adds (nerf_wgrad's and nerf_hashgrid_backward's convention: the caller zeroes them; the last
 * bits vary from run to run).  grad_weights / grad_biases are HOST arrays of n_hidden + 1 device pointers, shaped as the
 * parameters; each element may be NULL on its own.  A layer with both NULL gets no weight-gradient launch and nothing of it is touched.
 *
 * The two *_floats functions are the only source of the buffer sizes; they are pure host code (no GPU needed) and return -1 outside
 * the domain above.
 * Alignment: save and gsave 16 bytes (rows are moved as float4); every other pointer 4 bytes.  x rows are read as float4 when in_dim
 * is a multiple of 4 and x is 16-byte aligned, one float at a time otherwise: the values are the same.
 * Refused before any launch, with nerf_last_error set and nothing written: width, n_hidden, out_dim, in_dim or activation outside the
 * domain (NERF_ERR_UNSUPPORTED); B <= 0 (an empty batch is not a no-op here, as for nerf_hashgrid_*) or above the limit, null or
 * misaligned pointers, a null element of weights / biases (NERF_ERR_INVALID_ARG). */
int64_t nerf_fused_mlp_save_floats(int64_t B, int32_t width, int32_t n_hidden);
int64_t nerf_fused_mlp_grad_floats(int64_t B, int32_t width, int32_t n_hidden, int32_t out_dim);
int32_t nerf_fused_mlp_forward(const float* x, int64_t B, int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim,
                               int32_t activation, const float* const weights[], const float* const biases[], float* out,
                               float* save, void* stream);
int32_t nerf_fused_mlp_backward(const float* x, const float* out, const float* grad_out, int64_t B, int32_t in_dim, int32_t width,
                                int32_t n_hidden, int32_t out_dim, int32_t activation, const float* const weights[],
                                const float* save, float* gsave, float* const grad_weights[], float* const grad_biases[],
                                float* grad_x, void* stream);

/* ---- hash-grid radiance field: the ray-side glue ----------------------------------------------------------------
 * What runs between nerf_occupancy_mark / nerf_compact_valid, nerf_hashgrid_forward, nerf_fused_mlp_forward and nerf_composite when a
 * field  sigma, geo = sigma_net(hash(x)),  rgb = color_net(geo, SH(view direction))  is rendered along rays.  Entries were added to
 * this header without moving an existing contract: NERF_NN_ABI_VERSION stays 1.
 *
 * A POINT ID is ray * n_samples + sample, 0 <= id < n_points = n_rays * n_samples <= 2^31 - 1.  A call works on n_rows ROWS: row j is
 * the point  id = index ? index[j] : j  (index: device int32 [n_rows], ids as nerf_compact_valid leaves them, or NULL for the first
 * n_rows ids).  Arithmetic is fp32 with every operation separately rounded (fadd, fsub, fmul, div_rn, sqrt_rn: IEEE, round to nearest);
 * nothing is contracted.  No atomics: two runs write the same bytes.
 * Refused before any launch (NERF_ERR_INVALID_ARG, nothing written): n_rows <= 0 (an empty batch is not a no-op, as for
 * nerf_hashgrid_*), n_rows > n_points, n_rays <= 0, n_rays * n_samples > 2^31 - 1, n_samples outside [1, 192], a null required
 * pointer, a misaligned one.  Alignment: sh, geo, cin, g_cin, g_geo, raw, g_raw 16 bytes (rows are moved as float4); the others 4.
 * The kernels cannot check the ids of `index`; one outside [0, n_points) is never used as a store address (the scatter skips the
 * row, the gather reads zeros, the others read the last point).
 *
 * nerf_sh4_encode: rays_d [n_rays,3] -> sh [n_rays,16], the real spherical harmonics of degree 0..3 of the normalised direction:
 *     s = fadd(fadd(x*x, y*y), z*z),  r = sqrt_rn(s),  (x, y, z) = (div_rn(x, r), div_rn(y, r), div_rn(z, r))     (a*b: fmul)
 * then, every product and sum rounded, evaluated exactly as parenthesised, every constant rounded once to fp32:
 *     sh[0]  =  0.28209479177387814
 *     sh[1]  = -0.48860251190291987 * y           sh[2]  = 0.48860251190291987 * z           sh[3]  = -0.48860251190291987 * x
 *     sh[4]  = (1.0925484305920792 * x) * y       sh[5]  = (-1.0925484305920792 * y) * z
 *     sh[6]  = ((0.94617469575755997 * z) * z) - 0.31539156525251999
 *     sh[7]  = (-1.0925484305920792 * x) * z      sh[8]  = 0.54627421529603959 * ((x * x) - (y * y))
 *     sh[9]  = (0.59004358992664352 * y) * (((-3 * x) * x) + (y * y))
 *     sh[10] = ((2.8906114426405538 * x) * y) * z
 *     sh[11] = (0.45704579946446572 * y) * (1 - ((5 * z) * z))
 *     sh[12] = (0.3731763325901154 * z) * (((5 * z) * z) - 3)
 *     sh[13] = (0.45704579946446572 * x) * (1 - ((5 * z) * z))
 *     sh[14] = (1.4453057213202769 * z) * ((x * x) - (y * y))
 *     sh[15] = (0.59004358992664352 * x) * (((-x) * x) + ((3 * y) * y))
 * (orthonormal on the sphere).  A zero direction gives NaN, as the division says.
 *
 * nerf_field_points: the rows' positions, normalised into the box -> x [n_rows,3] in [0,1]:
 *     p = fadd(o[ray], fmul(d[ray], t))          t = tvals[ray * t_ray_stride + sample] (stride 0: one shared table); the two roundings
 *                                                of nerf_occupancy_mark, so a sample sits where the grid looked it up
 *     c = fminf(fmaxf(p, box_min), box_max)      per axis
 *     x = div_rn(fsub(c, box_min), extent)       ONE divisor for the three axes: extent = fp32(float64(largest axis extent of the fp32
 *                                                box) + 1e-6), computed by the caller and rounded once; must be > 0
 * (the arithmetic of hashgrid.normalize_to_bounds).  POINT MODE: rays_d == NULL and n_samples == 1 (anything else with a null rays_d is
 * refused): p = rays_o[id], tvals is not read; rays_o is then a list of n_rays points.  box_min and box_max are HOST arrays.
 *
 * nerf_field_color_inputs: the colour network's input rows and the rows' densities, from geo [n_rows,16] (the density network's
 * output) and sh [n_rays,16]:
 *     cin[j, 0:16] = geo[j, 0:16],   cin[j, 16:32] = sh[ray(id), 0:16],   sigma_rows[j] = geo[j, 0]            cin [n_rows,32]
 * nerf_field_color_inputs_backward: its adjoint with respect to geo, WRITTEN (not accumulated):
 *     g_geo[j, k] = g_cin[j, k] for 0 < k < 16,   g_geo[j, 0] = fadd(g_cin[j, 0], g_sigma_rows[j])
 * (sh does not depend on a parameter: it gets no gradient).
 *
 * nerf_field_raw_scatter: raw[id] = (rgb[j,0], rgb[j,1], rgb[j,2], sigma_rows[j]) for every row, one 16-byte store each, into
 * raw [n_points,4] -- nerf_composite's input.  Points not listed are not touched: the caller zero-fills raw, a culled sample has
 * raw = 0 (nerf_mlp_forward_rays_save_masked's convention).  rgb [n_rows,3], sigma_rows [n_rows].
 * nerf_field_raw_gather: the inverse read, g_rgb[j] = g_raw[id, 0:3], g_sigma_rows[j] = g_raw[id, 3], from nerf_composite_backward's
 * g_raw [n_points,4]. */
int32_t nerf_sh4_encode(const float* rays_d, int64_t n_rays, float* sh, void* stream);
int32_t nerf_field_points(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                          int32_t n_samples, const int32_t* index, int64_t n_rows, const float box_min[3], const float box_max[3],
                          float extent, float* x, void* stream);
int32_t nerf_field_color_inputs(const float* geo, const float* sh, const int32_t* index, int64_t n_rows, int64_t n_rays,
                                int32_t n_samples, float* cin, float* sigma_rows, void* stream);
int32_t nerf_field_color_inputs_backward(const float* g_cin, const float* g_sigma_rows, int64_t n_rows, float* g_geo, void* stream);
int32_t nerf_field_raw_scatter(const float* rgb, const float* sigma_rows, const int32_t* index, int64_t n_rows, int64_t n_points,
                               float* raw, void* stream);
int32_t nerf_field_raw_gather(const float* g_raw, const int32_t* index, int64_t n_rows, int64_t n_points, float* g_rgb,
                              float* g_sigma_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_NN_H */
