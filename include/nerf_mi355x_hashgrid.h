/* nerf_mi355x_hashgrid.h -- the deterministic, order-independent table gradient of the hash-grid encoding (libnerf_mi355x.so;
 * MI355X, gfx950).
 *
 * A fourth header of the same library.  nerf_mi355x.h keeps nerf_hashgrid_forward and nerf_hashgrid_backward,
 * whose table gradient is summed with fp32 atomics (the last bits depend on the arrival order); its table of entries is pinned by the
 * suite, so the entries below are additions and live here: neither NERF_ABI_VERSION nor NERF_NN_ABI_VERSION moves.  The conventions,
 * the level table (offsets_host, scales_host), the cell, the corner weights and the rows are those of nerf_hashgrid_backward:
 * device pointers to contiguous row-major fp32, caller-allocated outputs and workspace, the library owns no memory and does not
 * synchronise, calls only enqueue work on `stream`.
 *
 * THE ARITHMETIC.  A TERM is what nerf_hashgrid_backward adds: t = fmul(w, grad_out[b, l*C + c]) in fp32, w the corner weight
 * (1.0f times the factors in axis order), for every point b, level l, corner and channel c; its destination ELEMENT is
 * (offsets[l] + row) * C + c of grad_emb.  e(t) is the biased exponent field of t, 0 .. 255.  A NULL term has e(t) = 0 (zero or
 * subnormal): it contributes nothing.  A POISON term has e(t) = 255 (Inf or NaN).  The number of guard bits is
 *     K = min(30, 39 - ceil(log2(B * 2^D)))            (>= 4 for every accepted B and D)
 * Per element, over its terms:
 *     emax = max e(t)                                                                     (0 when it has none)
 *     for every live term (1 <= e(t) <= 254), provided emax < 255:
 *         m = the 24-bit significand of t with the hidden bit set,  s = emax - e(t)
 *         q = sign(t) * (s <= K ? m << (K - s) : m >> (s - K))     the right shift truncates the magnitude; 24 or more gives 0
 *     acc = sum q      in signed 64-bit two's complement; |q| <= (2^24 - 1) * 2^K and at most B * 2^D terms meet in one element, so
 *                      |acc| < 2^63 for every input: the accumulator cannot overflow
 *     emax == 0:    grad_emb[element] is neither read nor written
 *     emax == 255:  grad_emb[element] = quiet NaN (0x7fc00000)
 *     otherwise:    v = ldexpf(float_rn(acc), emax - 150 - K),   grad_emb[element] = fadd(grad_emb[element], v)
 * float_rn rounds the integer to fp32, to nearest even: the call's exact sum of the q, rounded once (a v in the subnormal range is
 * rounded once more by the scaling).  Integer maximum and integer addition are associative and commutative, so grad_emb is a function
 * of the MULTISET of terms: the same bytes from run to run and under any permutation of the points.  Against the exact sum of the
 * fp32 terms, v errs by the truncations, at most (number of terms) * 2^(emax - 150 - K), and by its one rounding.
 *
 * The workspace: acc, int64 [E], followed by emax, uint32 [E], with E = rows * C and rows = offsets[L] - offsets[0]:
 * 12 * E bytes rounded up to a multiple of 256, 16-byte aligned.  The entry zero-fills it itself, in stream order; its contents
 * afterwards are unspecified.
 */
#ifndef NERF_MI355X_HASHGRID_H
#define NERF_MI355X_HASHGRID_H

#include "nerf_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace for a table of `rows` rows of C floats.  Pure host.  -1 outside the domain: rows outside [1, 2^31 - 1], C not
 * in {1, 2, 4, 8}. */
int64_t nerf_hashgrid_deterministic_workspace_bytes(int64_t rows, int32_t C);

/* K above.  Pure host.  -1 outside the domain: D not in {2, 3, 4}, B < 1, B * D > 2^31 - 1. */
int32_t nerf_hashgrid_deterministic_guard_bits(int64_t B, int32_t D);

/* x [B,D], grad_out [B,L*C], grad_emb [offsets[L],C]: ACCUMULATES the table gradient of the call into grad_emb as written above (the
 * caller zeroes it, as for nerf_hashgrid_backward; elements no live term reaches are not touched).  The input gradient is not part
 * of this entry: nerf_hashgrid_backward with grad_emb = NULL writes it.
 * Refused before any launch, nothing written, nerf_last_error set: everything nerf_hashgrid_backward refuses for (B, D, C, L, the
 * level table); a null x, grad_out, grad_emb or workspace; grad_out not aligned to 4*C bytes, grad_emb not to 4, the workspace not
 * to 16 (NERF_ERR_INVALID_ARG); workspace_bytes below nerf_hashgrid_deterministic_workspace_bytes(offsets[L] - offsets[0], C)
 * (NERF_ERR_WORKSPACE). */
int32_t nerf_hashgrid_backward_deterministic(const float* x, const float* grad_out, int64_t B, int32_t D, int32_t C, int32_t L,
                                             const int32_t offsets_host[], const float scales_host[], float* grad_emb,
                                             void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_HASHGRID_H */
