// Hash-grid table gradient, deterministic and order-independent (DESIGN.md section 2.12.1; include/nerf_mi355x_hashgrid.h has the
// contract).  The same terms t = w * grad_out as nerf_hashgrid_grad_emb_kernel, summed exactly per table element in 64-bit fixed
// point (nerf_fixed_sum.h) instead of with fp32 atomics: three passes in stream order over a zero-filled workspace
//   exponent   emax[elem] = max over the element's terms of the biased exponent         no-return uint32 atomic max
//   add        acc[elem] += q(term, emax[elem])                                          no-return 64-bit integer atomic add
//   finish     grad_emb[elem] += value(acc[elem], emax[elem])                            one thread per element, plain loads and stores
// Integer max and add do not depend on the arrival order, so the bytes are the same from run to run and under any permutation of
// the points.  The first two passes keep the lane mapping of the fp32 kernel: one thread per (point, channel), channel fastest, one
// level per blockIdx.y, so the C lanes of a row form one contiguous segment of 4*C (emax) or 8*C (acc) bytes.  Both recompute
// the cell and the weights (cheap next to the atomics) and so form bit-identical terms.  No inline asm, no LDS.
#include "../../include/nerf_mi355x_hashgrid.h"
#include "nerf_host.h"
#include "nerf_fixed_sum.h"

namespace {

// the terms of thread (b, c) at level blockIdx.y: f(element relative to the first level's first row, bits of the fp32 term)
template <int D, int C, class F>
__device__ __forceinline__ void hg_det_terms(const float* __restrict__ x, const float* __restrict__ grad_out, uint32_t B, uint32_t L,
                                             const HgLevels& lv, F&& f) {
  const uint32_t t = blockIdx.x * kHgBlock + threadIdx.x;     // B*C < 2^31
  const uint32_t b = t / C, c = t % C;
  if (b >= B) return;
  const int l = blockIdx.y;
  const HgLevel<D> level(lv, l);
  const HgCell<D> cell(x + b * D, level.scale);
  const float go = grad_out[(b * L + l) * C + c];
  const size_t first = (size_t)(lv.offsets[l] - lv.offsets[0]) * C + c;
#pragma unroll
  for (int idx = 0; idx < (1 << D); ++idx) {
    uint32_t gc[D];
    const float w = cell.corner(idx, gc);
    f(first + (size_t)level.row(gc) * C, __float_as_uint(w * go));
  }
}

template <int D, int C>
__global__ __launch_bounds__(kHgBlock)
void nerf_hashgrid_det_exponent_kernel(const float* __restrict__ x, const float* __restrict__ grad_out, uint32_t B, uint32_t L,
                                       HgLevels lv, uint32_t* __restrict__ emax) {
  hg_det_terms<D, C>(x, grad_out, B, L, lv, [&](size_t elem, uint32_t bits) {
    const uint32_t e = fx_exponent(bits);
    if (e != 0u) atomicMax(emax + elem, e);                   // result unused: the no-return form; a null term asks for nothing
  });
}

template <int D, int C>
__global__ __launch_bounds__(kHgBlock)
void nerf_hashgrid_det_add_kernel(const float* __restrict__ x, const float* __restrict__ grad_out, uint32_t B, uint32_t L, HgLevels lv,
                                  int K, const uint32_t* __restrict__ emax, unsigned long long* __restrict__ acc) {
  hg_det_terms<D, C>(x, grad_out, B, L, lv, [&](size_t elem, uint32_t bits) {
    const uint32_t e = fx_exponent(bits);
    if (e == 0u || e == kFxPoison) return;
    const uint32_t top = emax[elem];                          // complete: the exponent pass ended before this kernel began
    if (top == kFxPoison) return;
    atomicAdd(acc + elem, (unsigned long long)fx_quantize(bits, top, K));     // two's complement; result unused
  });
}

__global__ __launch_bounds__(kHgBlock)
void nerf_hashgrid_det_finish_kernel(const unsigned long long* __restrict__ acc, const uint32_t* __restrict__ emax, uint64_t E, int K,
                                     float* __restrict__ grad_emb) {
  const uint64_t i = (uint64_t)blockIdx.x * kHgBlock + threadIdx.x;
  if (i >= E) return;
  const uint32_t top = emax[i];
  if (top == 0u) return;                                      // no live term: the element is neither read nor written
  grad_emb[i] = top == kFxPoison ? __uint_as_float(0x7fc00000u) : grad_emb[i] + fx_finish((int64_t)acc[i], top, K);
}

// elements and bytes of the workspace of a table of `rows` rows; -1 outside the domain
int64_t hg_det_workspace_bytes(int64_t rows, int32_t C) {
  if (rows < 1 || rows > 0x7fffffffLL || (C != 1 && C != 2 && C != 4 && C != 8)) return -1;
  return align256(12 * rows * C);
}

}  // namespace

extern "C" {

int64_t nerf_hashgrid_deterministic_workspace_bytes(int64_t rows, int32_t C) { return hg_det_workspace_bytes(rows, C); }

int32_t nerf_hashgrid_deterministic_guard_bits(int64_t B, int32_t D) {
  if (D < 2 || D > 4 || B < 1 || B > 0x7fffffffLL / D) return -1;
  return fx_guard_bits(B << D);
}

int32_t nerf_hashgrid_backward_deterministic(const float* x, const float* grad_out, int64_t B, int32_t D, int32_t C, int32_t L,
                                             const int32_t* offsets_host, const float* scales_host, float* grad_emb, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  const char* entry = "nerf_hashgrid_backward_deterministic";
  HgLevels lv;
  int rc = hg_check(entry, B, D, C, L, offsets_host, scales_host, lv);
  if (rc) return rc;
  if (!x || !grad_out || !grad_emb || !workspace) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!hg_aligned(grad_out, C) || !hg_aligned(grad_emb, 1) || ((uintptr_t)workspace & 15u) != 0)
    return fail(NERF_ERR_INVALID_ARG, "%s: grad_out must be aligned to 4*C bytes, grad_emb to 4 and the workspace to 16", entry);
  const int64_t rows = (int64_t)lv.offsets[L] - lv.offsets[0];
  if (workspace_bytes < hg_det_workspace_bytes(rows, C))
    return fail(NERF_ERR_WORKSPACE, "%s: the workspace is smaller than nerf_hashgrid_deterministic_workspace_bytes(rows, C)", entry);
  const uint64_t E = (uint64_t)rows * C;
  const int K = fx_guard_bits(B << D);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)workspace;   // int64 [E], then uint32 [E]
  uint32_t* emax = (uint32_t*)(acc + E);
  if (hipMemsetAsync(workspace, 0, (size_t)(12 * E), st) != hipSuccess) return fail(NERF_ERR_HIP, "%s: memset failed", entry);
  rc = hg_dispatch(D, C, [&](auto d, auto c) {
    int r = NERF_LAUNCH((nerf_hashgrid_det_exponent_kernel<decltype(d)::value, decltype(c)::value>), hg_grid(B * C, L), dim3(kHgBlock),
                        st, x, grad_out, (uint32_t)B, (uint32_t)L, lv, emax);
    if (r) return r;
    return NERF_LAUNCH((nerf_hashgrid_det_add_kernel<decltype(d)::value, decltype(c)::value>), hg_grid(B * C, L), dim3(kHgBlock), st, x,
                       grad_out, (uint32_t)B, (uint32_t)L, lv, K, (const uint32_t*)emax, acc);
  });
  if (rc) return rc;
  return NERF_LAUNCH(nerf_hashgrid_det_finish_kernel, hg_grid((int64_t)E, 1), dim3(kHgBlock), st, (const unsigned long long*)acc,
                     (const uint32_t*)emax, E, K, grad_emb + (size_t)lv.offsets[0] * C);
}

}  // extern "C"
