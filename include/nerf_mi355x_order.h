/* nerf_mi355x_order.h -- unit orders of the fp32 render MLP (libnerf_mi355x.so; MI355X, gfx950).
 *
 * A sixth header of the same library.  nerf_mi355x.h keeps nerf_pack_model; its table of entries is pinned by
 * the suite, so the entries below are additions and live here: NERF_ABI_VERSION does not move.  Conventions as there: device pointers
 * unless marked HOST, caller-allocated outputs, the library owns no memory and does not synchronise, calls with a `stream` only
 * enqueue work on it.
 *
 * WHY.  The fp32 inference kernels skip the MFMAs of a k-step whose activation register is zero in all 64 lanes: both units of the
 * pair {act_feat(t, r, 0), act_feat(t, r, 1)} are off at all 32 points of the tile.  Permuting the hidden units of a layer (rows of
 * W_l and b_l, the matching columns of whatever consumes h_l) gives the same network.  An ORDER places units that are off together
 * into one register, so more k-steps are skipped; the skip itself stays a run-time decision per tile and is exact for any order.
 *
 * AN ORDER TABLE is uint8_t order[8][256]: order[l][position] = the original unit of h_l (the output of pts_linears.l) that sits at
 * `position` of the permuted layer.  Every row must be a permutation of 0 .. 255 (not checked on the device: a row that is not
 * one packs some units twice and others never -- a wrong network, but no access outside the parameters).
 */
#ifndef NERF_MI355X_ORDER_H
#define NERF_MI355X_ORDER_H

#include "nerf_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nerf_pack_model(params, packed, NERF_PREC_F32, stream) for the network permuted by `order` (device, [8][256] uint8): the stream of
 * nerf_packed_model_bytes(NERF_PREC_F32) bytes in the unchanged layout, fold region included.  order[l] applies to the output index
 * and the bias of pts_linears.l, to the input index of pts_linears.(l+1) (the h-part of layer 5 for l = 4), and, for l = 7, to the
 * input side of feature_linear and to alpha_linear's weights.  The encodings' columns, feature_linear's outputs, the views layer,
 * the rgb head and the head biases are not permuted.  order == NULL: the bytes of nerf_pack_model.  Every inference entry takes the
 * result as its `packed`; raw differs from the identity stream's in the last bits only (the same 256 products per sum, added in
 * another order).  The SAVE entries and the backward chain expect the identity stream: their rows are in parameter order.
 * NERF_ERR_UNSUPPORTED for every precision but NERF_PREC_F32. */
int32_t nerf_pack_model_ordered(const float* const params[24], const uint8_t* order, void* packed, int32_t precision, void* stream);

/* Co-dead counts of a SAVE forward.  `save`: the buffer an fp32 SAVE forward that stores every row filled for n_points points
 * (nerf_mlp_forward_points_save, nerf_mlp_forward_rays_save; nerf_train_save_floats(n_points) floats, 16-byte aligned); only its
 * ReLU sign-bit blocks are read.  counts[l][i][j] (int32, [8][256][256], every element written): the number of 32-point tiles --
 * points 32 k .. 32 k + 31 as the render launches cut them; the ragged last tile counts with the points it has -- in which units i
 * and j of h_l are both off (<= 0 before the ReLU) at every point.  counts[l][i][i] is unit i's own count.  n_points >= 1. */
int32_t nerf_unit_order_stats(const float* save, int64_t n_points, int32_t* counts, void* stream);

/* One layer's order from its counts.  Pure HOST: counts[256 * 256] and order[256] are host arrays, no device is touched.  The rule
 * (csrc/nerf_unit_order_match.h): pairs i < j sorted by (count descending, i, j ascending), taken greedily while both units are free;
 * the 128 pairs sorted by (count descending, lower unit ascending) go to k-steps 0 .. 127, the lower unit into lane half 0.  Only
 * counts[i][j] with i < j are read; the result is a function of them alone, ties included, and always a permutation of 0 .. 255. */
int32_t nerf_unit_order_match(const int32_t counts[65536], int32_t order[256]);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_ORDER_H */
