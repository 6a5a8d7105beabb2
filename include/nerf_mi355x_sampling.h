/* nerf_mi355x_sampling.h -- where the samples of a hash-field ray lie: importance sampling from the field's own density and
 * stratified jitter, for any sample counts (libnerf_mi355x.so; MI355X, gfx950).
 *
 * One more header of the same library.  Every earlier header's table of entries is pinned by the suite, so
 * these entries are additions with a table of their own and no ABI version moves.  Conventions are those of nerf_mi355x_field.h:
 * device pointers to contiguous row-major fp32, caller-allocated outputs, calls only enqueue work on `stream`, the library owns no
 * memory and does not synchronise; fp32 with every operation separately rounded (fadd, fsub, fmul, div_rn), nothing contracted; no
 * atomics, so two runs write the same bytes.  Refused before any launch (NERF_ERR_INVALID_ARG, nothing written): a null required
 * pointer, a pointer that is not aligned to 4 bytes (raw: 16), counts outside the domain an entry states, a ray stride other than 0
 * or the row length.
 */
#ifndef NERF_MI355X_SAMPLING_H
#define NERF_MI355X_SAMPLING_H

#include "nerf_mi355x_field.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nerf_field_sample_importance: inverse-CDF resampling of a ray from the weights of a coarse pass.
 *   weights  [n_rays, Sc]   what nerf_composite writes as `weights` for the coarse depths (PRECONDITION: >= 0, so the cdf below does
 *                           not decrease; anything else, NaN included, moves samples but never an access outside the buffers)
 *   t_coarse                the coarse depths of ray r at t_coarse + r * t_ray_stride, t_ray_stride 0 (one table [Sc]) or Sc
 *                           (PRECONDITION: non-decreasing per ray)
 *   u                       the Sf numbers in [0, 1] of ray r at u + r * u_ray_stride, u_ray_stride 0 (one table [Sf]) or Sf; any order
 *   t_merged [n_rays, Sc + Sf]   the Sc coarse and the Sf fine depths of the ray, ascending
 *   t_fine   [n_rays, Sf]   nullable: the fine depths, t_fine[r, k] from u[r, k] (the caller's order)
 * Domain: Sc = n_coarse >= 3, Sf = n_fine >= 1, Sc + Sf <= 192, n_rays >= 1, n_rays * (Sc + Sf) <= 2^31 - 1.
 *
 * Per ray, with w = the ray's weights, t = its coarse depths and K = Sc - 2 (the first and the last weight are not used):
 *     w'_i   = fadd(w[i + 1], 1e-5f)                                   i = 0 .. K - 1
 *     total  = fadd(... fadd(fadd(w'_0, w'_1), w'_2) ..., w'_{K-1})    one lane per ray, left to right, starting from w'_0
 *     pdf_i  = div_rn(w'_i, total)
 *     cdf_0  = +0,   cdf_{i+1} = fadd(cdf_i, pdf_i)                    K + 1 values, the same sequential lane
 *     bins_j = fmul(0.5f, fadd(t[j + 1], t[j]))                        j = 0 .. K: K + 1 edges, the midpoints of the coarse depths
 * and for every u of the ray
 *     inds   = #{m in [0, K] : cdf_m <= u},   below = clamp(inds - 1, 0, K),   above = clamp(inds, 0, K)
 *     denom  = fsub(cdf[above], cdf[below]),  replaced by 1 where denom < 1e-5f
 *     frac   = div_rn(fsub(u, cdf[below]), denom)
 *     fine   = fadd(bins[below], fmul(frac, fsub(bins[above], bins[below])))
 * A fine depth is a function of its u alone, so t_merged depends only on the multiset of the ray's u: it is the ascending sort of the
 * Sc + Sf values (equal values are the same bits, so the sort has one result).  u >= cdf_K gives bins_K exactly (below = above = K,
 * denom = 1, the last factor is 0); every fine depth lies in [bins_0, bins_K].
 *
 * How this departs from nerf_sample_fine_rays (nerf_mi355x.h), which is cut to the reference's 64 + 128:
 *   the clamp      `above` is clamped to K, not to K - 1: the last bin [bins_{K-1}, bins_K] is reachable (there, u beyond cdf_{K-1}
 *                  collapses onto bins_{K-1}, the reference's behaviour);
 *   the sum order  `total` is the plain left-to-right sum above, not torch.sum's vector order on a 62-element row;
 *   the input      the contract starts at the WEIGHTS, not at the raw densities: the entry contains no exp, and the CPU restatement
 *                  (tests/hashfield_sampling_reference.py) is bit for bit; no fast_sampling masks, no adjoint.
 * One lane per ray, 64 rays per workgroup, each ray's row staged in LDS and the merged rows written back coalesced. */
int32_t nerf_field_sample_importance(const float* weights, const float* t_coarse, int64_t t_ray_stride, const float* u,
                                     int64_t u_ray_stride, int64_t n_rays, int32_t n_coarse, int32_t n_fine, float* t_merged,
                                     float* t_fine, void* stream);

/* nerf_field_stratified_depths: nerf_stratified_samples for any S = n_samples in [1, 192].  t_table [S] (one table), jitter
 * [n_rays, S] -> t [n_rays, S]:
 *     lower_s = s == 0 ? t_table[0] : fmul(0.5f, fadd(t_table[s], t_table[s - 1]))
 *     upper_s = s == S - 1 ? t_table[S - 1] : fmul(0.5f, fadd(t_table[s + 1], t_table[s]))
 *     t[r, s] = fadd(lower_s, fmul(fsub(upper_s, lower_s), jitter[r, s]))
 * bit-equal to the CPU torch expression  mids = 0.5 * (t[1:] + t[:-1]); lower = cat(t[:1], mids); upper = cat(mids, t[-1:]);
 * lower + (upper - lower) * jitter.  S == 1 gives t_table[0].  n_rays >= 1, n_rays * S <= 2^31 - 1. */
int32_t nerf_field_stratified_depths(const float* t_table, const float* jitter, int64_t n_rays, int32_t n_samples, float* t,
                                     void* stream);

/* nerf_field_density_scatter: the `raw` of a density-only pass.  Row j of `sigma` (sigma[j * sigma_stride]; sigma_stride >= 1 floats:
 * 16 for column 0 of the density network's output [n_rows,16]) goes to point id = index ? index[j] : j as
 *     raw[id] = (0, 0, 0, sigma_j)                  raw [n_points,4], one 16-byte store
 * nerf_field_raw_scatter without the [n_rows,3] of colours: nerf_composite's `weights` read the density column alone.  Points the list
 * leaves out are not touched (the caller zero-fills); an id outside [0, n_points) is skipped, never a store address.
 * 1 <= n_rows <= n_points <= 2^31 - 1. */
int32_t nerf_field_density_scatter(const float* sigma, int64_t sigma_stride, const int32_t* index, int64_t n_rows, int64_t n_points,
                                   float* raw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355X_SAMPLING_H */
