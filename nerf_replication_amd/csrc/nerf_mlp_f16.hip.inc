// Fused positional-encoding + NeRF MLP with fp16 activations/weights and fp32 accumulation on
// v_mfma_f32_32x32x16_f16 (BASELINE config 5).//
// Same replaced reference lines as nerf_mlp_f32.hip.inc (network.py:199-258, :49-74, freq.py:31-32;
// in ray mode volume_renderer.py:63/:267/:314).  Not the parity path: tolerance is PSNR-based.
//
// Structure (gfx950, 16x the fp32 MFMA rate, so operand feeding and VALU work now matter):
//  * workgroup = 8 waves (2 per SIMD, <=256 VGPRs each, no AGPR shuffling), each wave owns 32 points;
//    the partner wave's MFMAs cover a wave's epilogue VALU (ReLU + cvt_pk) and LDS reads.
//  * activations stay in registers as packed fp16 B fragments: 16 k-steps x 4 VGPRs (X) ping-pong
//    with Y; out-tiles are produced one at a time (m-outer, k-inner): acc 16 regs -> 8 packed regs.
//  * weights: one stream of 1-KiB A fragments in consumption order (nerf_layout.h), staged by
//    LDS-DMA (global_load_lds_dwordx4) in 32-KiB chunks through a 4-slot LDS ring shared by the
//    8 waves: per chunk each wave issues 4 DMAs, three chunks are always in flight, one
//    `s_waitcnt vmcnt(8)` + `s_barrier` per chunk (every 32 MFMAs per wave).  L2 -> LDS traffic is
//    1 KiB per 8 MFMAs, LDS -> VGPR 1 KiB per MFMA per wave (ds_read_b128, conflict-free).
//  * persistent workgroups (one per CU): the stream wraps around from tile to tile, so the ring
//    never drains; biases live in a 16-KiB LDS const region loaded once.
//  * positional encoding by exact base sincos + angle doubling (fp32 error 2^k * 6e-8 << fp16 ulp).
//  * sigma and rgb heads are 1-out-tile MFMA layers (rows 0 / 0..2), so (r,g,b,sigma) of point p end
//    up in registers 0..2 / 0 of lane p: one float4 store, no cross-lane traffic.

#include "nerf_mlp_common.h"

constexpr int kF16DmaPerWave = nerf::kF16ChunkFrags / kF16Waves;                            // 4

// timing-only switches (tools/ab_bench.py builds variants with -D...)
#ifndef NERF_F16_HACK_NOADV
#define NERF_F16_HACK_NOADV 0       // timing-only: never advance the LDS ring (wrong results)
#endif
#ifndef NERF_F16_HACK_NOBARRIER
#define NERF_F16_HACK_NOBARRIER 0
#endif
#ifndef NERF_F16_HACK_NORELU
#define NERF_F16_HACK_NORELU 0      // timing-only: no ReLU on the packed outputs
#endif
#ifndef NERF_F16_HACK_NOEPI
#define NERF_F16_HACK_NOEPI 0       // timing-only: no bias / fp16 pack / ReLU after an out-tile (wrong results)
#endif
// A-fragment prefetch ring in registers (4 VGPRs per slot); fragments in flight ahead of the consumer (may reach into the next chunk)
constexpr int kPfRing = 4, kPfDist = 3;

struct FragRing {
  const char* gsrc;        // (wave-uniform) byte address of (chunk 0, this wave's first fragment): stays in SGPRs
  unsigned lane_off;       // + this lane's 16 bytes
  lds_char* ldst;          // LDS address of this wave's first fragment in slot 0 (wave-uniform)
  const lds_char* ring;    // LDS ring base (slot 0, fragment 0) + lane*16
  const lds_char* lcur;    // this lane's address of fragment 0 of the chunk being consumed
  const lds_char* lnext;   // ... of the chunk after it (already landed: prefetch may run into it)
  int cur_slot;            // ring slot of the chunk being consumed
  int next_chunk;          // stream chunk the next DMA fetches (wraps at kF16Chunks)
  int next_slot;           // ring slot the next DMA fills
  bool dens;               // density-only instance: the stream wraps after the chunk that starts with the sigma head
  h8 pf[kPfRing];
};
// density-only chunk sequence: L0..L7 (chunks 0..29), the chunk that starts with the sigma head (30), then chunk 0 again
constexpr int kF16ChunkSigma = nerf::kF16FragSigma / nerf::kF16ChunkFrags;
static_assert(nerf::kF16FragSigma % nerf::kF16ChunkFrags == 0, "the sigma head starts a chunk");

__device__ __forceinline__ void ring_issue(FragRing& r) {
  const char* src = r.gsrc + (long long)r.next_chunk * nerf::kF16ChunkBytes;
  lds_char* dst = r.ldst + r.next_slot * nerf::kF16ChunkBytes;
#pragma unroll
  for (int i = 0; i < kF16DmaPerWave; ++i)
    __builtin_amdgcn_global_load_lds((gbl_void*)((src + i * nerf::kF16FragBytes) + r.lane_off),
                                     (lds_void*)(dst + i * nerf::kF16FragBytes), 16, 0, 0);
  int nc = r.next_chunk + 1;
  if (nc == (r.dens ? kF16ChunkSigma + 1 : nerf::kF16Chunks)) nc = 0;
  r.next_chunk = nc;
  r.next_slot = (r.next_slot + 1) & (kF16RingSlots - 1);
}

__device__ __forceinline__ void ring_set_slots(FragRing& r) {
  r.lcur = r.ring + r.cur_slot * nerf::kF16ChunkBytes;
  r.lnext = r.ring + ((r.cur_slot + 1) & (kF16RingSlots - 1)) * nerf::kF16ChunkBytes;
}

// End of chunk c (its last fragment has been consumed by this wave).  Ring state: c+1 landed (it
// was waited for one chunk ago, so fragment prefetch already runs into it), c+2 and c+3 in flight.
//   vmcnt(4): my DMAs of c+2 have landed (only c+3's four remain)  -> after the barrier c+2 is
//   readable by everyone, and everyone is done with c, whose slot is refilled with c+4.
// LDS reads still in flight here are prefetches of c+1 only, so no lgkmcnt wait is needed.
__device__ __forceinline__ void ring_advance(FragRing& r) {
  __builtin_amdgcn_sched_barrier(0);       // keep the MFMA that consumed the last fragment above
#if NERF_F16_HACK_NOBARRIER            // timing-only: the DMA protocol without the workgroup barrier (racy: wrong results possible)
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
#else
  asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
#endif
  __builtin_amdgcn_sched_barrier(0);
  ring_issue(r);
  r.cur_slot = (r.cur_slot + 1) & (kF16RingSlots - 1);
  ring_set_slots(r);
}

__device__ __forceinline__ h8 frag_read(const FragRing& r, int pfi) {   // pfi in [0, 64): static
  const lds_char* base = pfi < nerf::kF16ChunkFrags ? r.lcur : r.lnext;
  return *reinterpret_cast<lds_ch8*>(base + (pfi & (nerf::kF16ChunkFrags - 1)) * nerf::kF16FragBytes);
}

// acc(m) = sum_s A(frag) * B[s], B = [B1 (KS1 k-steps), B2 (KS2 k-steps)]; the accumulator starts
// from 0 and the bias is added in the epilogue: its four LDS reads are issued a few k-steps before
// the end of the tile, so no out-tile ever starts behind an LDS round trip.
// F0 = fragment index (mod 32) at which this layer starts inside a chunk.
template <int KS1, int KS2, int F0, bool WITH_BIAS>
__device__ __forceinline__ f32x16 gemm16_tile(FragRing& r, int m, const h8* B1, const h8* B2,
                                              lds_cfloat* bias_lds_h) {
  constexpr int KS = KS1 + KS2;
  constexpr int kBiasAt = KS > 6 ? KS - 6 : 0;
  static_assert(nerf::kF16ChunkFrags % kPfRing == 0, "ring phase must be static");
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  f32x4 bq0, bq1, bq2, bq3;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int fi = (F0 + m * KS + s) & (nerf::kF16ChunkFrags - 1);
    r.pf[(fi + kPfDist) % kPfRing] = frag_read(r, fi + kPfDist);
    if (WITH_BIAS && s == kBiasAt) {
      lds_cf32x4* b = reinterpret_cast<lds_cf32x4*>(bias_lds_h + m * 16);
      bq0 = b[0]; bq1 = b[1]; bq2 = b[2]; bq3 = b[3];
    }
    __builtin_amdgcn_sched_barrier(0x406);     // VALU/SALU/TRANS may cross; LDS reads and MFMAs keep this order
    acc = mfma16(r.pf[fi % kPfRing], s < KS1 ? B1[s] : B2[s - KS1], acc);
    if (fi == nerf::kF16ChunkFrags - 1 && !NERF_F16_HACK_NOADV) ring_advance(r);
  }
  if (WITH_BIAS) {
    acc[0] += bq0.x; acc[1] += bq0.y; acc[2] += bq0.z; acc[3] += bq0.w;
    acc[4] += bq1.x; acc[5] += bq1.y; acc[6] += bq1.z; acc[7] += bq1.w;
    acc[8] += bq2.x; acc[9] += bq2.y; acc[10] += bq2.z; acc[11] += bq2.w;
    acc[12] += bq3.x; acc[13] += bq3.y; acc[14] += bq3.z; acc[15] += bq3.w;
  }
  return acc;
}

// The same k-loop with the bias already IN the accumulator it starts from (`acc`), and the next out-tile's accumulator
// filled from LDS on the way (`nxt` <- next_bias, 16 floats = four ds_read_b128 landing directly in accumulator
// registers, issued six k-steps before the end).  The per-tile epilogue loses its 16 v_add_f32: measured with
// profiles/collect_variants.sh the epilogue VALU (add + pack + ReLU) was 18 % of the kernel AND what pulled the clock
// down (2.10 GHz without it, 1.77 with).
template <int KS1, int KS2, int F0>
__device__ __forceinline__ f32x16 gemm16_tile_b(FragRing& r, int m, const h8* B1, const h8* B2, f32x16 acc,
                                                lds_cfloat* next_bias, f32x16& nxt) {
  constexpr int KS = KS1 + KS2;
  constexpr int kBiasAt = KS > 6 ? KS - 6 : 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int fi = (F0 + m * KS + s) & (nerf::kF16ChunkFrags - 1);
    r.pf[(fi + kPfDist) % kPfRing] = frag_read(r, fi + kPfDist);
    if (s == kBiasAt && next_bias != nullptr) {
      lds_cf32x4* b = reinterpret_cast<lds_cf32x4*>(next_bias);
      const f32x4 q0 = b[0], q1 = b[1], q2 = b[2], q3 = b[3];
      nxt[0] = q0.x; nxt[1] = q0.y; nxt[2] = q0.z; nxt[3] = q0.w; nxt[4] = q1.x; nxt[5] = q1.y; nxt[6] = q1.z; nxt[7] = q1.w;
      nxt[8] = q2.x; nxt[9] = q2.y; nxt[10] = q2.z; nxt[11] = q2.w; nxt[12] = q3.x; nxt[13] = q3.y; nxt[14] = q3.z; nxt[15] = q3.w;
    }
    __builtin_amdgcn_sched_barrier(0x406);     // VALU/SALU/TRANS may cross; LDS reads and MFMAs keep this order
    acc = mfma16(r.pf[fi % kPfRing], s < KS1 ? B1[s] : B2[s - KS1], acc);
    if (fi == nerf::kF16ChunkFrags - 1 && !NERF_F16_HACK_NOADV) ring_advance(r);
  }
  return acc;
}

// Full layer: NM out-tiles -> packed fp16 B fragments OUT[2*NM], optional ReLU.  `carry` enters holding the bias of
// this layer's out-tile 0 and leaves holding `next_layer_bias` (out-tile 0 of the layer that follows; nullptr: unused).
template <int KS1, int KS2, int NM, int F0>
__device__ __forceinline__ void gemm16_layer(FragRing& r, lds_cfloat* bias_lds_h, const h8* B1, const h8* B2,
                                             h8* OUT, bool relu, f32x16& carry, lds_cfloat* next_layer_bias) {
#pragma unroll
  for (int m = 0; m < NM; ++m) {
#if !NERF_F16_HACK_NOEPI
    f32x16 nxt;
    const f32x16 acc = gemm16_tile_b<KS1, KS2, F0>(r, m, B1, B2, carry, m + 1 < NM ? bias_lds_h + (m + 1) * 16 : next_layer_bias, nxt);
    carry = nxt;
#else
    const f32x16 acc = gemm16_tile<KS1, KS2, F0, !NERF_F16_HACK_NOEPI>(r, m, B1, B2, bias_lds_h);
#endif
    h8 o0, o1;
    if (NERF_F16_HACK_NOEPI) {          // keep the data dependence, drop the arithmetic
      f32x4 a0 = {acc[0], acc[1], acc[2], acc[3]}, a1 = {acc[8], acc[9], acc[10], acc[11]};
      OUT[2 * m] = __builtin_bit_cast(h8, a0);
      OUT[2 * m + 1] = __builtin_bit_cast(h8, a1);
      continue;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { o0[j] = (_Float16)acc[j]; o1[j] = (_Float16)acc[8 + j]; }
    if (relu && !NERF_F16_HACK_NORELU) {
      o0 = __builtin_elementwise_max(o0, (h8)(_Float16)0);
      o1 = __builtin_elementwise_max(o1, (h8)(_Float16)0);
    }
    OUT[2 * m] = o0;
    OUT[2 * m + 1] = o1;
  }
}
__device__ __forceinline__ f32x16 bias_tile(lds_cfloat* bias) {        // one exposed LDS round trip (once per 256-point tile)
  lds_cf32x4* b = reinterpret_cast<lds_cf32x4*>(bias);
  const f32x4 q0 = b[0], q1 = b[1], q2 = b[2], q3 = b[3];
  f32x16 a;
  a[0] = q0.x; a[1] = q0.y; a[2] = q0.z; a[3] = q0.w; a[4] = q1.x; a[5] = q1.y; a[6] = q1.z; a[7] = q1.w;
  a[8] = q2.x; a[9] = q2.y; a[10] = q2.z; a[11] = q2.w; a[12] = q3.x; a[13] = q3.y; a[14] = q3.z; a[15] = q3.w;
  return a;
}

// DENS: stop after the sigma head (MlpArgs::density_only), raw = (0, 0, 0, sigma).  DSKIP (MlpArgs::skip_dead_colour): a WAVE whose
// 32 points all have sigma <= 0 -- weight exactly 0 in compositing -- skips the fragment reads, MFMAs and epilogues of the
// colour branch and writes rgb = 0; it still takes part in the ring protocol (its DMA share and the chunk barriers), which is
// what paces it.  The matrix pipe of its SIMD is then the partner wave's alone, and the kernel is power-bound (section 2.1b).
template <bool RAY_MODE, bool DENS = false, bool DSKIP = false>
__global__ __launch_bounds__(kF16Threads)
void nerf_mlp_f16_kernel(MlpArgs a) {
  static_assert(!(DENS && DSKIP), "dead-colour skipping is a variant of the full network");
  using namespace nerf;
  __shared__ __attribute__((aligned(16))) char smem_generic[kF16LdsBytes];
  lds_char* smem = (lds_char*)smem_generic;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5;
  const char* packed = reinterpret_cast<const char*>(a.packed);
  if (a.index && *a.count <= 0) return;               // masked pass with nothing to do (uniform: before any DMA/barrier)

  // ---- const region (biases) + first three chunks by LDS-DMA -------------------------------
  {
    const char* csrc = packed + wave * 2048 + lane * 16;
    lds_char* cdst = smem + wave * 2048;
    __builtin_amdgcn_global_load_lds((gbl_void*)csrc, (lds_void*)cdst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void*)(csrc + 1024), (lds_void*)(cdst + 1024), 16, 0, 0);
  }
  FragRing r;
  r.gsrc = packed + kF16ConstBytes + wave * (kF16DmaPerWave * kF16FragBytes); r.lane_off = (unsigned)lane * 16u;
  r.ldst = smem + kF16ConstBytes + wave * (kF16DmaPerWave * kF16FragBytes);
  r.ring = smem + kF16ConstBytes + lane * 16;
  r.cur_slot = 0; r.next_chunk = 0; r.next_slot = 0; r.dens = DENS;
  ring_issue(r); ring_issue(r); ring_issue(r);
  // const region + chunks 0 and 1 landed (chunk 2 in flight), visible to all waves; then chunk 3
  asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  ring_issue(r);
  ring_set_slots(r);
#pragma unroll
  for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);

  lds_cfloat* cst = reinterpret_cast<lds_cfloat*>(smem);
  lds_cfloat* bias_h = cst + kF16OffBias + h * 128;            // + 256 per layer
  lds_cfloat* bias_views_h = cst + kF16OffBiasViews + h * 64;

  const long long n_points = a.index ? (long long)*a.count : a.n_points;   // masked pass: device-side count
  const long long n_tiles = (n_points + kF16TilePts - 1) / kF16TilePts;

  // point + unit view direction of this lane for a workgroup tile (indices clamped to the last point)
  auto load_point = [&](long long tile, float& x0, float& x1, float& x2, float& d0, float& d1, float& d2) {
    long long p = tile * kF16TilePts + wave * 32 + (lane & 31);
    if (p >= n_points) p = n_points - 1;
    if (p < 0) p = 0;
    if (a.index) p = a.index[p];
    const long long ray = p / a.n_samples;
    const int s_idx = (int)(p - ray * a.n_samples);
    if (RAY_MODE) {
      const float t = a.tvals[ray * a.t_ray_stride + s_idx];
      d0 = a.rays_d[ray * 3 + 0]; d1 = a.rays_d[ray * 3 + 1]; d2 = a.rays_d[ray * 3 + 2];
      x0 = a.rays_o[ray * 3 + 0] + d0 * t; x1 = a.rays_o[ray * 3 + 1] + d1 * t; x2 = a.rays_o[ray * 3 + 2] + d2 * t;
    } else {
      x0 = a.pts[p * 3 + 0]; x1 = a.pts[p * 3 + 1]; x2 = a.pts[p * 3 + 2];
    }
    if (a.viewdirs != nullptr) {
      d0 = a.viewdirs[ray * 3 + 0]; d1 = a.viewdirs[ray * 3 + 1]; d2 = a.viewdirs[ray * 3 + 2];
    } else {
      const float inv = 1.0f / __fsqrt_rn(d0 * d0 + d1 * d1 + d2 * d2);
      d0 *= inv; d1 *= inv; d2 *= inv;
    }
  };
  // positional encodings straight into B fragments (slot n = 8*kstep + elem, nerf_layout.h):
  // exact base sincos (octave 0 for lane-half 0, octave 5 resp. 2 for lane-half 1) + angle doubling
  h8 PE[4];
  auto encode_xyz = [&](float x0, float x1, float x2) {
    const float hs = h ? 32.0f : 1.0f;
    const float xs[3] = {x0, x1, x2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float sv, cv;
      sincos_cw(xs[c] * hs, sv, cv);
#pragma unroll
      for (int ko = 0; ko < 5; ++ko) {
        const int n = 2 * (3 * ko + c);
        PE[n >> 3][n & 7] = (_Float16)sv;
        PE[(n + 1) >> 3][(n + 1) & 7] = (_Float16)cv;
        const float s2 = 2.0f * sv * cv, c2 = fmaf(-2.0f * sv, sv, 1.0f);
        sv = s2; cv = c2;
      }
    }
    PE[3][6] = (_Float16)(h ? x2 : x0);
    PE[3][7] = (_Float16)(h ? 0.0f : x1);
  };

  h8 DPE[2];
  auto encode_dir = [&](float q0, float q1, float q2) {
    {
    const float ds = h ? 4.0f : 1.0f;
    const float dd[3] = {q0, q1, q2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float sv, cv;
      sincos_cw(dd[c] * ds, sv, cv);
#pragma unroll
      for (int ko = 0; ko < 2; ++ko) {
        const int n = 2 * (3 * ko + c);
        DPE[n >> 3][n & 7] = (_Float16)sv;
        DPE[(n + 1) >> 3][(n + 1) & 7] = (_Float16)cv;
        const float s2 = 2.0f * sv * cv, c2 = fmaf(-2.0f * sv, sv, 1.0f);
        sv = s2; cv = c2;
      }
    }
    DPE[1][4] = (_Float16)(h ? q2 : q0);
    DPE[1][5] = (_Float16)(h ? 0.0f : q1);
    DPE[1][6] = (_Float16)0.0f; DPE[1][7] = (_Float16)0.0f;
  }
  };

  // software pipeline across tiles: a tile's rays are loaded, and its xyz encoding computed, during
  // the previous tile (under that tile's later layers)
  float dc0, dc1, dc2;
  {
    float x0, x1, x2;
    load_point(blockIdx.x, x0, x1, x2, dc0, dc1, dc2);
    encode_xyz(x0, x1, x2);
  }
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    float xn0, xn1, xn2, dn0, dn1, dn2;
    load_point(tile + gridDim.x, xn0, xn1, xn2, dn0, dn1, dn2);                  // lands during L0..L5

    h8 X[16], Y[16];
    f32x16 carry = bias_tile(bias_h);                                            // bias of (L0, out-tile 0)
    gemm16_layer<4, 0, 8, 0>(r, bias_h, PE, PE, X, true, carry, bias_h + 256);   // L0
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {                                            // L1..L4
      gemm16_layer<16, 0, 8, 0>(r, bias_h + (1 + 2 * it) * 256, X, X, Y, true, carry, bias_h + (2 + 2 * it) * 256);
      gemm16_layer<16, 0, 8, 0>(r, bias_h + (2 + 2 * it) * 256, Y, Y, X, true, carry, bias_h + (3 + 2 * it) * 256);
    }
    gemm16_layer<4, 16, 8, 0>(r, bias_h + 5 * 256, PE, X, Y, true, carry, bias_h + 6 * 256);   // L5 = skip(PE) + hidden
    gemm16_layer<16, 0, 8, 0>(r, bias_h + 6 * 256, Y, Y, X, true, carry, bias_h + 7 * 256);    // L6
    gemm16_layer<16, 0, 8, 0>(r, bias_h + 7 * 256, X, X, Y, true, carry, DENS ? nullptr : bias_h + 8 * 256);    // L7 -> Y = relu(h7)
    const f32x16 sig = gemm16_tile<16, 0, 0, false>(r, 0, Y, Y, bias_h);           // sigma head on relu(h7)
    f32x16 col;
    bool dead_wave = false;                                                        // (wave-uniform)
    if constexpr (DSKIP)
      dead_wave = __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(
                      h == 0 && tile * kF16TilePts + wave * 32 + (lane & 31) < n_points &&
                      sig[0] + cst[kF16OffHeadBias + 3] > 0.0f) != 0ull)) == 0;
    if constexpr (DENS) {
      // density only (the coarse pass of a hierarchical render: the reference reads nothing but sigma of it,
      // volume_renderer.py:335): the stream wraps after this chunk; its other 16 fragments (the start of the feature layer)
      // are skipped by advancing the ring by hand, and the register prefetch is re-primed on the next tile's first
      // fragments (one exposed LDS round trip per 256-point tile)
      ring_advance(r);
#pragma unroll
      for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);
#pragma unroll
      for (int i = 0; i < 16; ++i) col[i] = 0.0f;
      encode_xyz(xn0, xn1, xn2);
    } else if (dead_wave) {
      // (wave-uniform) no point of this wave has density: the colour branch's 208 fragments (16 left in this chunk + 6
      // chunks) go by unread -- seven chunk ends, each with this wave's DMA share and the workgroup barrier
#pragma unroll 1
      for (int c = 0; c < 7; ++c) ring_advance(r);
#pragma unroll
      for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);
#pragma unroll
      for (int i = 0; i < 16; ++i) col[i] = 0.0f;
      encode_xyz(xn0, xn1, xn2);
    } else {
    gemm16_layer<16, 0, 8, 16>(r, bias_h + 8 * 256, Y, Y, X, false, carry, bias_views_h);      // feature (no ReLU); carry <- views bias
    h8 V[8];
    __builtin_amdgcn_sched_barrier(0);
    encode_dir(dc0, dc1, dc2);
    encode_xyz(xn0, xn1, xn2);      // next tile's encoding: here only X (the feature vector) is live, so the
                                    // sincos temporaries fit (placed after layer 5 they spilled ~70 VGPRs per tile)
    gemm16_layer<16, 2, 4, 16>(r, bias_views_h, X, DPE, V, true, carry, nullptr);   // views: [feature, dirs] -> 128
    col = gemm16_tile<8, 0, 24, false>(r, 0, V, V, bias_h);                        // rgb head
    }

    const long long pl = tile * kF16TilePts + wave * 32 + (lane & 31);
    if (pl < n_points && h == 0) {
      const long long p = a.index ? (long long)a.index[pl] : pl;
      f32x4 out;
      // (a skipped colour branch leaves col = 0 and must give rgb = 0, not the bias)
      const bool no_colour = DENS || dead_wave;
      out.x = no_colour ? 0.0f : col[0] + cst[kF16OffHeadBias + 0];
      out.y = no_colour ? 0.0f : col[1] + cst[kF16OffHeadBias + 1];
      out.z = no_colour ? 0.0f : col[2] + cst[kF16OffHeadBias + 2];
      out.w = sig[0] + cst[kF16OffHeadBias + 3];
      reinterpret_cast<f32x4*>(a.raw)[p] = out;
    }
    dc0 = dn0; dc1 = dn1; dc2 = dn2;
  }
  // no LDS-DMA may still be in flight when the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
