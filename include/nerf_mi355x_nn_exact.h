/* nerf_mi355x_nn_exact.h -- the exact, order-independent weight and bias gradients of the fused MLP (libnerf_mi355x.so; MI355X,
 * gfx950).
 *
 * A fifth header of the same library.  nerf_mi355x_nn.h keeps nerf_fused_mlp_forward and
 * nerf_fused_mlp_backward, whose parameter gradients are summed with fp32 atomics (the last bits depend on the arrival order); its
 * table of entries is pinned by the suite, so the entries below are additions and live here: neither NERF_ABI_VERSION nor
 * NERF_NN_ABI_VERSION moves.  The network, the layouts of x, out, save, gsave, weights, grad_weights and grad_biases, the domain, the
 * alignments and the conventions are those of nerf_fused_mlp_backward: device pointers to contiguous row-major fp32, caller-allocated
 * outputs and workspace, the library owns no memory and does not synchronise, calls only enqueue work on `stream`.
 *
 * THE ARITHMETIC.  Layer i has dz_i [B,n_out] (block i of gsave) and input rows in_i [B,n_in] (in_0 = x, in_i = h_{i-1}, block
 * i - 1 of save).  Per column, over the B rows, as the UNSIGNED maximum of the bit patterns with the sign cleared (exact, order-
 * independent; a NaN outranks Inf and survives):
 *     A[o] = max_p |dz_i[p,o]|          H[k] = max_p |in_i[p,k]|
 * e(v) is the biased exponent field of v, 0 .. 255.  A NULL term has e = 0 (zero or subnormal) and contributes nothing; ReLU zeros
 * in h and in dz make null terms.  The number of guard bits is
 *     K = min(30, 39 - ceil(log2(B)))                         (>= 16 for every accepted B)
 * Weight gradient, element (o,k):  the terms are t_p = fmul(dz_i[p,o], in_i[p,k]), one fp32 multiplication each, rounded to
 *     nearest, not contracted into anything;  emax = e(fmul(A[o], H[k])).  Rounding is monotonic, so e(t_p) <= emax for every p.
 * Bias gradient, element o:  the terms are t_p = dz_i[p,o];  emax = e(A[o]).
 * Per element, provided 1 <= emax <= 254, over its live terms (1 <= e(t) <= 254):
 *         m = the 24-bit significand of t with the hidden bit set,  s = emax - e(t)
 *         q = sign(t) * (s <= K ? m << (K - s) : m >> (s - K))     the right shift truncates the magnitude; 24 or more gives 0
 *     acc = sum q      in signed 64-bit two's complement; |q| <= (2^24 - 1) * 2^K and an element has at most B terms, so
 *                      |acc| < 2^63 for every input: the accumulator cannot overflow
 *     emax == 0:    the gradient element is neither read nor written
 *     emax == 255:  the gradient element = quiet NaN (0x7fc00000)
 *     otherwise:    v = ldexpf(float_rn(acc), emax - 150 - K),   element = fadd(element, v)
 * (nerf_hashgrid_backward_deterministic's arithmetic, with one difference: the scale comes from the column maxima and not from the
 * element's largest term, so no pass over the B * n_out * n_in products is needed only to find it.)  Integer maximum and addition
 * are associative and commutative: the gradients are a function of the MULTISET of rows, the same bytes from run to run and under
 * any permutation of the rows.  Two consequences of the column-maximum scale:
 *     TRUNCATION UNIT.  What the right shifts lose is at most (number of terms) * 2^(emax - 150 - K): relative to A[o] * H[k], not to
 *     the element's largest term.  Against the real-number sum,
 *         |v - truth| <= 2^-24 * sum_p |dz * in|  +  B * 2^(emax - 150 - K)  +  2^-24 * |truth|
 *     (term formation, truncation, the final rounding; the first part is absent for a bias).
 *     FALSE POISON.  An element whose column maxima multiply to 2^128 or more (or are Inf and 0) is set to NaN even if no single term
 *     overflows.  Inputs of that size are outside anything a gradient clip or an optimizer handles.
 *
 * The workspace: int64 accumulators, per layer its weights [n_out * n_in] then its bias [n_out], in layer order; behind them the
 * uint32 column maxima of x [in_dim], of the save blocks [n_hidden * width] and of the gsave blocks [n_hidden * width + out_dim];
 * rounded up to a multiple of 256 bytes, 16-byte aligned.  The entry zero-fills it itself, in stream order; its contents afterwards
 * are unspecified.
 */
#ifndef NERF_MI355X_NN_EXACT_H
#define NERF_MI355X_NN_EXACT_H

#include "nerf_mi355x_nn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace.  Pure host.  -1 outside nerf_fused_mlp_*'s domain (in_dim 1..256, width 64 or 128, n_hidden 1..8,
 * out_dim 1..16). */
int64_t nerf_fused_mlp_exact_workspace_bytes(int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim);

/* K above.  Pure host.  -1 outside the domain: B < 1 or B > 8 388 607. */
int32_t nerf_fused_mlp_exact_guard_bits(int64_t B);

/* nerf_fused_mlp_backward with exact sums: the SAME chain kernel writes gsave and grad_x (their bytes are the default entry's), then
 * grad_weights[i] and grad_biases[i] ACCUMULATE the call's gradients as written above (the caller zeroes them, as for
 * nerf_fused_mlp_backward), for exactly the layers and kinds whose pointer is not NULL; nothing of a layer with both NULL is touched.
 * Refused before any launch, nothing written, nerf_last_error set: everything nerf_fused_mlp_backward refuses; a null workspace or
 * one not aligned to 16 bytes (NERF_ERR_INVALID_ARG); workspace_bytes below nerf_fused_mlp_exact_workspace_bytes(in_dim, width,
 * n_hidden, out_dim) (NERF_ERR_WORKSPACE). */
int32_t nerf_fused_mlp_backward_exact(const float* x, const float* out, const float* grad_out, int64_t B, int32_t in_dim, int32_t width,
                                      int32_t n_hidden, int32_t out_dim, int32_t activation, const float* const weights[],
                                      const float* save, float* gsave, float* const grad_weights[], float* const grad_biases[],
                                      float* grad_x, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_NN_EXACT_H */
