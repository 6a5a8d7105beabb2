/* nerf_mi355x_nn.h -- small-network entries of libnerf_mi355x.so: a fused ReLU MLP on fp32 MFMA (MI355X, gfx950).
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

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_NN_H */
