/* nerf_mi355x_deform.h -- the rank-factorised deformation field of a dynamic scene (libnerf_mi355x.so; MI355X, gfx950).
 *
 * One more header of the same library.  The field warps the normalised position of every sample before the hash
 * grid is looked up: DNeRFNGP of the reference's hashencoder/hashgrid.py.  Its parameters are three tables feat[i], i = 0..2, each
 * [3, F, T, R] fp32 (plane axis j, channel f, frame, position), F = 64, T = num_frames, R = reso, and
 *     delta_i(x, t) = sum_f  v_0(f) * v_1(f) * v_2(f),      v_j(f) = bilinear(feat[i][j, f]; x_j, t).
 * Conventions are those of nerf_mi355x_field.h: device pointers to contiguous row-major fp32, caller-allocated outputs, calls only
 * enqueue work on `stream`, the library owns no memory; fp32 with every operation separately rounded (fadd, fsub, fmul), nothing
 * contracted.  Row j is the point  id = index ? index[j] : j,  its ray is  id / n_samples;  a row whose id lies outside
 * [0, n_rays * n_samples) is SKIPPED: nothing is read or written for it, the id never becomes an address.
 *
 * THE DEVICE LAYOUT OF THE TABLES.  The parameters keep a channel's 64 values T * R floats apart.  The kernels read `packed`, one
 * buffer of 9 * T * R * 64 floats, channel innermost:
 *     packed[(((i * 3 + j) * T + y) * R + c) * 64 + f] = feat[i][((j * 64 + f) * T + y) * R + c]
 * so that one tap of one plane is one 256-byte row: a wave with lane = channel reads it in one request and adds its gradient back as
 * one 256-byte atomic wave-instruction.  nerf_deform_pack makes it, nerf_deform_unpack_grad brings a gradient in that layout back to
 * the parameters' shape; both only move bits.  `packed` and `g_packed` must be aligned to 256 bytes.
 *
 * THE ARITHMETIC of a row with position x = (x_0, x_1, x_2) (PRECONDITION: every x_j in [0, 1], the output of nerf_field_points) and
 * frame number t = time[ray]:
 *     tc = fminf(fmaxf(t, 0), T - 1),    y0 = min((int)floorf(tc), T - 2),    wy = fsub(tc, y0),    uy = fsub(1, wy)
 *     per axis j:   ix = fmul(x_j, R - 1),   x0 = max(0, min((int)floorf(ix), R - 2)),   wx = fsub(ix, x0),   ux = fsub(1, wx)
 * (grid_sample(align_corners = True) with every tap in range; the rows are indexed by the frame number itself).  A position outside
 * [0, 1] or NaN gives an unspecified value, never an address outside the tables (x0 is clamped on both sides).  With
 * a00 = P[y0][x0], a01 = P[y0][x0 + 1], a10 = P[y0 + 1][x0], a11 = P[y0 + 1][x0 + 1] of the plane P = feat[i][j, f]:
 *     v_j(f) = fadd(fmul(fadd(fmul(a00, ux), fmul(a01, wx)), uy),  fmul(fadd(fmul(a10, ux), fmul(a11, wx)), wy))
 *     p(f)   = fmul(fmul(v_0(f), v_1(f)), v_2(f))
 *     delta_i = the sum of p(0..63), folded in six steps:  p[f] = fadd(p[f], p[f + h]) for f < h,   h = 32, 16, 8, 4, 2, 1;   p[0]
 *     x'_i   = fminf(fmaxf(fadd(x_i, delta_i), 0), 1)
 * A NaN t: delta and x' of the row are NaN, and the row adds nothing to any gradient.
 * THE CANONICAL FRAME: a ray with t == 0 (either sign of zero) gets x' = x, the same bits, and g_x_warped of its rows reaches no
 * table.  delta is the field's value at frame 0 all the same: it is what the smoothness loss penalises.
 *
 * THE TABLE GRADIENT of a row, from g' = g_x_warped[row] and gd = g_delta[row] (each optional), per output axis i:
 *     s = fadd(x_i, delta_i);   g = (t != 0 && s >= 0 && s <= 1) ? g'_i : +0      (torch.clamp's rule: equality passes, NaN does not)
 *     g = fadd(g, gd_i)          when g_delta is given
 * everything recomputed from x and the tables as above (the forward saves nothing).  If g is exactly zero, nothing is added for this i;
 * otherwise, per plane j with (a, b) the other two axes, a < b, and per channel f:
 *     q = fmul(g, fmul(v_a(f), v_b(f)));    qt = fmul(q, uy);    qb = fmul(q, wy)
 *     G[a00] += fmul(qt, ux),   G[a01] += fmul(qt, wx),   G[a10] += fmul(qb, ux),   G[a11] += fmul(qb, wx)
 * with fp32 atomic adds into g_packed, which the caller has zeroed (the entry ACCUMULATES; the order of the adds is not fixed, so two
 * runs may differ in the last bits).  The gradients with respect to x and to time are not computed.
 *
 * Refused before any launch (NERF_ERR_INVALID_ARG, nothing written): F != 64, T < 2, R < 2, 9 * T * R * 64 > 2^31 - 1; n_rows <= 0,
 * n_rows > n_rays * n_samples, n_rays <= 0, n_rays * n_samples > 2^31 - 1, n_samples outside [1, 192]; a null required pointer; a
 * misaligned one (packed, g_packed: 256 bytes, the others 4); the forward without an output, the backward without an input gradient.
 */
#ifndef NERF_MI355X_DEFORM_H
#define NERF_MI355X_DEFORM_H

#include "nerf_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nerf_deform_packed_bytes: the bytes of `packed` (and of g_packed), 9 * T * R * 64 * 4; -1 outside the domain above.  Pure host. */
int64_t nerf_deform_packed_bytes(int32_t n_channels, int32_t n_frames, int32_t reso);

/* nerf_deform_table_bytes: the bytes of ONE parameter table feat[i], 3 * 64 * T * R * 4; -1 outside the domain.  Pure host. */
int64_t nerf_deform_table_bytes(int32_t n_channels, int32_t n_frames, int32_t reso);

/* nerf_deform_pack: feat[0..2] (HOST array of three device pointers, each [3, 64, T, R]) -> packed, the layout above. */
int32_t nerf_deform_pack(const float* const feat[3], int32_t n_channels, int32_t n_frames, int32_t reso, float* packed, void* stream);

/* nerf_deform_unpack_grad: g_packed (the layout above) -> g_feat[0..2] (HOST array of three device pointers, each [3, 64, T, R]);
 * every element of the three is WRITTEN (not accumulated) with the bits of its element of g_packed. */
int32_t nerf_deform_unpack_grad(const float* g_packed, int32_t n_channels, int32_t n_frames, int32_t reso, float* const g_feat[3],
                                void* stream);

/* nerf_deform_forward: x [n_rows,3], time [n_rays], index (nullable) [n_rows] -> x_warped [n_rows,3] and delta [n_rows,3] (each
 * nullable, one at least).  A canonical row without `delta` reads no table. */
int32_t nerf_deform_forward(const float* x, const float* time, const int32_t* index, int64_t n_rows, int64_t n_rays, int32_t n_samples,
                            const float* packed, int32_t n_channels, int32_t n_frames, int32_t reso, float* x_warped, float* delta,
                            void* stream);

/* nerf_deform_backward: the same inputs, g_x_warped [n_rows,3] and g_delta [n_rows,3] (each nullable, one at least) -> adds the
 * table gradient into g_packed [9 * T * R * 64]. */
int32_t nerf_deform_backward(const float* x, const float* time, const int32_t* index, int64_t n_rows, int64_t n_rays,
                             int32_t n_samples, const float* packed, int32_t n_channels, int32_t n_frames, int32_t reso,
                             const float* g_x_warped, const float* g_delta, float* g_packed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_DEFORM_H */
