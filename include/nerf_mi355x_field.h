/* nerf_mi355x_field.h -- the spatial adjoint of the hash-grid radiance field's ray-side glue (libnerf_mi355x.so; MI355X, gfx950).
 *
 * A third header of the same library.  nerf_mi355x_nn.h keeps the forward glue of the field and its parameter
 * adjoints, and its table of 11 entries is pinned by the suite; the entries that carry a gradient back to the POSITIONS and to the
 * RAYS are additions and live here, so that neither NERF_NN_ABI_VERSION nor any existing contract moves.  Conventions, the point ids
 * and the rows (row j is the point  id = index ? index[j] : j) are those of nerf_mi355x_nn.h, "the ray-side glue": device pointers to
 * contiguous row-major fp32, caller-allocated outputs, calls only enqueue work on `stream`; fp32 with every operation separately
 * rounded (fadd, fsub, fmul, div_rn, sqrt_rn), nothing contracted; no atomics, so two runs write the same bytes.
 * Refused before any launch (NERF_ERR_INVALID_ARG, nothing written): n_rows <= 0, n_rows > n_points, n_rays <= 0,
 * n_rays * n_samples > 2^31 - 1, n_samples outside [1, 192], a null required pointer, a misaligned one (seed, g_cin, g_sh: 16 bytes,
 * the others 4), point mode with n_samples != 1 or with a per-ray output.  An id of `index` outside [0, n_points) is never used as a
 * store address.
 *
 * THE RUN OF A RAY, and the order of every per-ray sum below.  Ray r owns the rows whose id lies in [r * S, r * S + S), S = n_samples.
 * PRECONDITION: `index` is ASCENDING, as nerf_compact_valid leaves it; the rows of a ray are then one run [a, b) of row numbers,
 * a = the first row with id >= r * S and b = the first row with id >= r * S + S, both found by binary search over the n_rows ids
 * (index == NULL: a = min(r * S, n_rows), b = min(r * S + S, n_rows)).  A list that is not ascending gives sums over other rows, never
 * an access outside the buffers.  One wave of 64 lanes per ray.  Lane l starts at +0 and adds the terms of rows a + l, a + l + 64,
 * a + l + 128, ... (ascending) with one fadd each; then the 64 partial sums v[0..63] are folded in six steps,
 *     v[l] = fadd(v[l], v[l + h])  for l < h,     h = 32, 16, 8, 4, 2, 1,
 * and v[0] is the sum (an xor butterfly: fadd commutes, so every lane holds the same bits).  A ray without rows gets exactly +0.
 */
#ifndef NERF_MI355X_FIELD_H
#define NERF_MI355X_FIELD_H

#include "nerf_mi355x_nn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nerf_field_density_seed: the grad_out of nerf_fused_mlp_backward that means "the gradient of the raw density", seed [n_rows,16]:
 *     seed[j, 0] = (positive_only && !(sigma_j > 0)) ? 0 : 1,     seed[j, 1..15] = 0,     sigma_j = sigma[j * sigma_stride]
 * sigma_stride (floats, >= 1): 1 for a list sigma_rows [n_rows], 16 for column 0 of the density network's output [n_rows,16].  A NaN
 * density counts as not positive.  1 <= n_rows <= 2^31 - 1. */
int32_t nerf_field_density_seed(const float* sigma, int64_t sigma_stride, int64_t n_rows, int32_t positive_only, float* seed,
                                void* stream);

/* nerf_field_points_backward: the adjoint of nerf_field_points; its arguments, then g_x [n_rows,3], the gradient with respect to the
 * normalised positions.  Per row, p is recomputed with the forward's two roundings, p = fadd(o, fmul(d, t)) (point mode: p = o), and
 *     g_p[a] = (p[a] >= box_min[a] && p[a] <= box_max[a]) ? div_rn(g_x[j, a], extent) : +0          per axis a
 * (torch.clamp's rule: equality passes, NaN does not; one correctly rounded division by the forward's extent).
 * g_p (nullable): by_id == 0: row j is written at g_p[j] (g_p [n_rows,3], the compact layout); by_id != 0: at g_p[id] (g_p
 * [n_points,3], the layout nerf_composite_normals reads; points not listed are not touched, a row whose id is outside [0, n_points) is
 * skipped).
 * g_rays_o, g_rays_d [n_rays,3] (each nullable; rays only -- refused in point mode): per ray and axis, over the ray's run in the
 * order written down above,
 *     g_rays_o = sum g_p,     g_rays_d = sum fmul(t, g_p),  then  g_rays_d = fadd(g_rays_d, g_rays_d_view[ray])  if g_rays_d_view
 * is given ([n_rays,3], nerf_sh4_encode_backward's output; needs g_rays_d): g_rays_d is written once, as nerf_rays_backward writes it.
 * At least one of the three outputs must be given. */
int32_t nerf_field_points_backward(const float* rays_o, const float* rays_d, const float* tvals, int64_t t_ray_stride, int64_t n_rays,
                                   int32_t n_samples, const int32_t* index, int64_t n_rows, const float box_min[3],
                                   const float box_max[3], float extent, const float* g_x, const float* g_rays_d_view, int32_t by_id,
                                   float* g_p, float* g_rays_o, float* g_rays_d, void* stream);

/* nerf_field_sh_gradient: the adjoint of nerf_field_color_inputs with respect to sh: g_sh [n_rays,16], per ray and column k the sum
 * of g_cin[j, 16 + k] (g_cin [n_rows,32]) over the ray's run, in the order written down above.  Exactly +0 for a ray without rows. */
int32_t nerf_field_sh_gradient(const float* g_cin, const int32_t* index, int64_t n_rows, int64_t n_rays, int32_t n_samples,
                               float* g_sh, void* stream);

/* nerf_sh4_encode_backward: the adjoint of nerf_sh4_encode: rays_d [n_rays,3], g_sh [n_rays,16] (g_k = g_sh[ray, k]) ->
 * g_rays_d_view [n_rays,3].  s, r = sqrt_rn(s) and the unit direction (x, y, z) are recomputed as the forward computes them, and
 * q = 1 - ((5 * z) * z),  m = (y * y) - (x * x).  First the polynomial adjoint g_u, every product and sum rounded, each bracket
 * evaluated as parenthesised (c * v: the constant rounded once to fp32), the terms added left to right starting from the first:
 *     g_u.x =  g3 * -0.48860251190291987            + g4 * (1.0925484305920792 * y)           + g7 * (-1.0925484305920792 * z)
 *            + g8 * ((0.54627421529603959 * x) * 2)  + g9 * (((0.59004358992664352 * x) * y) * -6)
 *            + g10 * ((2.8906114426405538 * y) * z)  + g13 * (0.45704579946446572 * q)
 *            + g14 * (((1.4453057213202769 * x) * z) * 2)                                     + g15 * ((0.59004358992664352 * m) * 3)
 *     g_u.y =  g1 * -0.48860251190291987            + g4 * (1.0925484305920792 * x)           + g5 * (-1.0925484305920792 * z)
 *            + g8 * ((0.54627421529603959 * y) * -2) + g9 * ((0.59004358992664352 * m) * 3)
 *            + g10 * ((2.8906114426405538 * x) * z)  + g11 * (0.45704579946446572 * q)
 *            + g14 * (((1.4453057213202769 * y) * z) * -2)                                    + g15 * (((0.59004358992664352 * x) * y) * 6)
 *     g_u.z =  g2 * 0.48860251190291987             + g5 * (-1.0925484305920792 * y)          + g6 * ((0.94617469575755997 * z) * 2)
 *            + g7 * (-1.0925484305920792 * x)        + g10 * ((2.8906114426405538 * x) * y)
 *            + g11 * (((0.45704579946446572 * y) * z) * -10)
 *            + g12 * (0.3731763325901154 * (((15 * z) * z) - 3))
 *            + g13 * (((0.45704579946446572 * x) * z) * -10)                                  + g14 * (1.4453057213202769 * ((x * x) - (y * y)))
 * then the normalisation u = d / r:
 *     w = fadd(fadd(x * g_u.x, y * g_u.y), z * g_u.z),     g_rays_d_view[a] = div_rn(fsub(g_u[a], fmul(u[a], w)), r)
 * so that g_rays_d_view . rays_d = 0 up to rounding.  A zero direction gives NaN, as in the forward. */
int32_t nerf_sh4_encode_backward(const float* rays_d, const float* g_sh, int64_t n_rays, float* g_rays_d_view, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_FIELD_H */
