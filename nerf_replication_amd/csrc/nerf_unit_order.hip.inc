// Unit orders of the fp32 render MLP (DESIGN.md section 2.1.1; include/nerf_mi355x_order.h has the contract): the co-dead counts of a
// SAVE forward (nerf_unit_order_stats) and the host matching that turns a layer's counts into its order (nerf_unit_order_match,
// nerf_unit_order_match.h).  The ordered pack itself is nerf_pack_model_ordered in nerf_pack.hip.inc.
#include "../../include/nerf_mi355x_order.h"
#include "nerf_host.h"
#include "nerf_mlp_common.h"
#include "nerf_unit_order_match.h"

namespace {

// Reads the ReLU sign-bit blocks of TrainSave (1 KiB per 32-point tile and layer: lane (p, h), bit 16 (t & 1) + r of word t >> 1 <->
// unit act_feat(t, r, h) > 0; the idle lanes of a ragged last tile repeat its last point), never the activation rows: 9 KiB per tile
// instead of 8 x 32 KiB.  Workgroup (rb, layer) counts rows 32 rb .. 32 rb + 31 of the layer's matrix, thread j its column j.  Four
// tiles per round: each wave ORs one tile's block over the 32 points of either lane half (the 256 "on" bits of the tile) and leaves
// them in LDS; then every thread adds, for its column and each of the four tiles, the row units that are off with it.  Plain
// integer counts into registers, one store per element: no atomics, the same bytes every run.
__global__ __launch_bounds__(256) void nerf_unit_order_stats_kernel(const float* __restrict__ save, long long n_points,
                                                                    int32_t* __restrict__ counts) {
  using namespace nerf;
  const int rb = blockIdx.x, layer = blockIdx.y, j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const long long n_tiles = TrainSave::pad32(n_points) / kTilePts;
  const u32x4* bits = reinterpret_cast<const u32x4*>(save + TrainSave::off_bits(n_points));
  __shared__ unsigned on[4][2][4];                 // [tile of the round][lane half][word]
  // where unit u = 32 t + w sits: lane half (w >> 2) & 1, register (w & 3) + 4 (w >> 3)  (the inverse of act_feat)
  const int jt = j >> 5, jh = (j >> 2) & 1, jr = (j & 3) + 4 * ((j & 31) >> 3);
  int32_t cnt[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) cnt[i] = 0;
  for (long long t0 = 0; t0 < n_tiles; t0 += 4) {
    const long long tile = t0 + wave;
    u32x4 m = {~0u, ~0u, ~0u, ~0u};               // a tile past the end: every unit on, nothing is counted
    if (tile < n_tiles) m = bits[(tile * TrainSave::kMasked + layer) * 64 + lane];
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) {           // (d < 32: stays inside the lane half)
      m.x |= __shfl_xor(m.x, d); m.y |= __shfl_xor(m.y, d); m.z |= __shfl_xor(m.z, d); m.w |= __shfl_xor(m.w, d);
    }
    if ((lane & 31) == 0) {
      unsigned* dst = on[wave][lane >> 5];
      dst[0] = m.x; dst[1] = m.y; dst[2] = m.z; dst[3] = m.w;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const bool off_j = ((on[w][jh][jt >> 1] >> (16 * (jt & 1) + jr)) & 1u) == 0u;
      const unsigned off0 = ~on[w][0][rb >> 1] >> (16 * (rb & 1)), off1 = ~on[w][1][rb >> 1] >> (16 * (rb & 1));
      if (off_j) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const int r = (i & 3) + 4 * (i >> 3);
          cnt[i] += (int32_t)((((i >> 2) & 1 ? off1 : off0) >> r) & 1u);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 32; ++i) counts[((long long)layer * kHidden + 32 * rb + i) * kHidden + j] = cnt[i];
}

}  // namespace

extern "C" {

int32_t nerf_unit_order_stats(const float* save, int64_t n_points, int32_t* counts, void* stream) {
  if (n_points < 1 || n_points > 0x7fffffffLL * 32) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_unit_order_stats: bad size");
  if (!save || !counts) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_unit_order_stats: null argument");
  if (((uintptr_t)save & 15) != 0) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_unit_order_stats: save must be 16-byte aligned");
  return NERF_LAUNCH(nerf_unit_order_stats_kernel, dim3(8, 8), dim3(256), (hipStream_t)stream, save, (long long)n_points, counts);
}

int32_t nerf_unit_order_match(const int32_t counts[65536], int32_t order[256]) {
  if (!counts || !order) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_unit_order_match: null argument");
  nerf::unit_order_match(counts, order);
  return NERF_OK;
}

}  // extern "C"
