// The fp16-activation MLP (nerf_mlp_f16.hip.inc) on the OTHER matrix-core shape, v_mfma_f32_16x16x32_f16 -- precision
// NERF_PREC_F16S.  Same replaced reference lines, same arithmetic class (fp16 operands, fp32 accumulate; only the order of the
// fp32 partial sums inside a k-step differs), same LDS-DMA fragment ring, same 8-wave workgroups of 32 points per wave, same
// 1-KiB A fragment per 16 384 MACs -- so the two kernels are an A/B of the MFMA shape at equal output tile per wave and equal
// LDS bytes per FLOP (round-2 VERDICT item 3; MI355X_MICROARCH.md "DVFS give-back" item 7: on random data the chip holds a
// higher clock on the 16x16x32 loop).  Layout: nerf_layout.h "f16s".
// Needs nerf_mlp_f16.hip.inc ahead of it (FragRing and its protocol).
//
// What changes with the shape:
//  * a wave's 32 points are two column groups of 16 (points 16n + c, lane = (c, g)); every A fragment feeds two MFMAs;
//  * an out-tile is 16 features: 4 accumulator registers per group; two consecutive out-tiles make one k-step fragment of
//    the next layer (8 fp16 per lane), again without any data movement;
//  * a lane evaluates 16 of the 64 encoding slots of BOTH of its points (the 32x32 kernel: 32 slots of one point): octaves
//    2g, 2g+1 by one exact sincos + one angle doubling, octaves 8, 9 and the raw coordinates as two per-lane-selected extras;
//  * biases are read in natural order (16m + 4g), straight into both groups' accumulators.

#include "nerf_mlp_common.h"

__device__ __forceinline__ f32x4 mfma16s(h8 a, h8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// one out-tile (16 features) for both point groups.  `cinit` holds the tile's bias (or 0): it is the C operand of the FIRST MFMA of
// both groups' chains (D != C), so the two accumulators need no copy of it; the NEXT tile's bias is fetched from LDS into `nxt` on
// the way (one ds_read_b128 landing in accumulator registers: no VALU for the bias at all)
template <int KS1, int KS2, int F0>
__device__ __forceinline__ void gemm16s_tile(FragRing& r, int m, const h8* B1a, const h8* B1b, const h8* B2a, const h8* B2b,
                                             const f32x4& cinit, f32x4& acc0, f32x4& acc1, lds_cfloat* next_bias, f32x4& nxt) {
  constexpr int KS = KS1 + KS2;
  constexpr int kBiasAt = KS > 5 ? KS - 5 : 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int fi = (F0 + m * KS + s) & (nerf::kF16ChunkFrags - 1);
    r.pf[(fi + kPfDist) % kPfRing] = frag_read(r, fi + kPfDist);
    if (s == kBiasAt && next_bias != nullptr) nxt = *reinterpret_cast<lds_cf32x4*>(next_bias);
    __builtin_amdgcn_sched_barrier(0x406);     // VALU/SALU/TRANS may cross; LDS reads and MFMAs keep this order
    const h8 w = r.pf[fi % kPfRing];
    acc0 = mfma16s(w, s < KS1 ? B1a[s] : B2a[s - KS1], s == 0 ? cinit : acc0);
    acc1 = mfma16s(w, s < KS1 ? B1b[s] : B2b[s - KS1], s == 0 ? cinit : acc1);
    if (fi == nerf::kF16ChunkFrags - 1) ring_advance(r);
  }
}

// Full layer: NM out-tiles of 16 features -> NM/2 packed fp16 B fragments per point group, optional ReLU.  `c` enters holding the
// bias of this layer's out-tile 0 and leaves holding that of the layer that follows (next_layer_bias; nullptr: left undefined).
template <int KS1, int KS2, int NM, int F0>
__device__ __forceinline__ void gemm16s_layer(FragRing& r, lds_cfloat* bias_g, const h8* B1a, const h8* B1b, const h8* B2a,
                                              const h8* B2b, h8* OUTa, h8* OUTb, bool relu, f32x4& c, lds_cfloat* next_layer_bias) {
  static_assert(NM % 2 == 0, "two out-tiles make one k-step of the next layer");
  f32x4 k0, k1;                                   // the even tile of a pair, waiting for its partner
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    f32x4 a0, a1, nx;
    gemm16s_tile<KS1, KS2, F0>(r, m, B1a, B1b, B2a, B2b, c, a0, a1, m + 1 < NM ? bias_g + 16 * (m + 1) : next_layer_bias, nx);
    c = nx;
    if ((m & 1) == 0) { k0 = a0; k1 = a1; continue; }
    h8 oa, ob;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      oa[j] = (_Float16)k0[j]; oa[4 + j] = (_Float16)a0[j];
      ob[j] = (_Float16)k1[j]; ob[4 + j] = (_Float16)a1[j];
    }
    if (relu) {
      oa = __builtin_elementwise_max(oa, (h8)(_Float16)0);
      ob = __builtin_elementwise_max(ob, (h8)(_Float16)0);
    }
    OUTa[m >> 1] = oa;
    OUTb[m >> 1] = ob;
  }
}

// DENS / DSKIP: as nerf_mlp_f16_kernel (density-only coarse pass; waves without density skip the colour branch)
template <bool RAY_MODE, bool DENS = false, bool DSKIP = false>
__global__ __launch_bounds__(kF16Threads)
void nerf_mlp_f16s_kernel(MlpArgs a) {
  static_assert(!(DENS && DSKIP), "dead-colour skipping is a variant of the full network");
  using namespace nerf;
  __shared__ __attribute__((aligned(16))) char smem_generic[kF16LdsBytes];
  lds_char* smem = (lds_char*)smem_generic;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, g = lane >> 4;
  const char* packed = reinterpret_cast<const char*>(a.packed);
  if (a.index && *a.count <= 0) return;               // masked pass with nothing to do (uniform: before any DMA/barrier)

  // ---- const region (biases) + first three chunks by LDS-DMA
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
  asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");      // const region + chunks 0 and 1 landed
  __builtin_amdgcn_sched_barrier(0);
  ring_issue(r);
  ring_set_slots(r);
#pragma unroll
  for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);

  lds_cfloat* cst = reinterpret_cast<lds_cfloat*>(smem);
  lds_cfloat* bias_g = cst + kF16sOffBias + 4 * g;              // + 256 per layer, + 16 per out-tile
  lds_cfloat* bias_views_g = cst + kF16sOffBiasViews + 4 * g;

  const long long n_points = a.index ? (long long)*a.count : a.n_points;   // masked pass: device-side count
  const long long n_tiles = (n_points + kF16TilePts - 1) / kF16TilePts;

  // the lane's two points of a workgroup tile (indices clamped to the last point): positions x[n][3] and unit view directions
  // d[n][3], loaded SEPARATELY and late: x of the NEXT tile and d of THIS tile are both fetched at the start of layer 7 (their
  // latency hides under its 256 MFMAs), so nothing of either is live through the trunk (with the loads at the top of the tile
  // the kernel spilled 17 registers per lane and tile)
  auto point_of = [&](long long tile, int n, long long& ray, int& s_idx) -> long long {
    long long p = tile * kF16TilePts + wave * 32 + 16 * n + col;
    if (p >= n_points) p = n_points - 1;
    if (p < 0) p = 0;
    if (a.index) p = a.index[p];
    ray = p / a.n_samples;
    s_idx = (int)(p - ray * a.n_samples);
    return p;
  };
  auto load_x = [&](long long tile, float (&x)[2][3]) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      long long ray; int s_idx;
      const long long p = point_of(tile, n, ray, s_idx);
      if (RAY_MODE) {
        const float t = a.tvals[ray * a.t_ray_stride + s_idx];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[n][c] = a.rays_o[ray * 3 + c] + a.rays_d[ray * 3 + c] * t;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) x[n][c] = a.pts[p * 3 + c];
      }
    }
  };
  auto load_d = [&](long long tile, float (&d)[2][3]) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      long long ray; int s_idx;
      point_of(tile, n, ray, s_idx);
      if (a.viewdirs != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[n][c] = a.viewdirs[ray * 3 + c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[n][c] = a.rays_d[ray * 3 + c];
        const float inv = 1.0f / __fsqrt_rn(d[n][0] * d[n][0] + d[n][1] * d[n][1] + d[n][2] * d[n][2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[n][c] *= inv;
      }
    }
  };
  // encodings straight into B fragments (nerf_layout.h pe16s_*): ONE instruction stream for the four lane groups, which differ
  // in per-lane scales and selects only
  h8 PE[2][2];
  auto encode_xyz = [&](const float (&x)[2][3]) {
    const float sg = g == 0 ? 1.0f : g == 1 ? 4.0f : g == 2 ? 16.0f : 64.0f;          // octave 2g
    const float s0 = g < 2 ? 256.0f : 512.0f, s1 = g == 0 ? 256.0f : 512.0f;           // extras: octave 8 or 9
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sv, cv;
        sincos_cw(x[n][c] * sg, sv, cv);
        PE[n][0][2 * c] = (_Float16)sv;                 // pair c: slots 2c, 2c+1 (octave 2g)
        PE[n][0][2 * c + 1] = (_Float16)cv;
        const float s2 = 2.0f * sv * cv, c2 = fmaf(-2.0f * sv, sv, 1.0f);             // pair 3+c: slots 6+2c, 7+2c (octave 2g+1)
        const int n2 = 6 + 2 * c;
        PE[n][n2 >> 3][n2 & 7] = (_Float16)s2;
        PE[n][(n2 + 1) >> 3][(n2 + 1) & 7] = (_Float16)c2;
      }
      const float e0 = g == 0 ? x[n][0] : g == 1 ? x[n][2] : x[n][1];
      const float e1 = g == 0 ? x[n][1] : g == 1 ? x[n][0] : x[n][2];
      float sa, ca, sb, cb;
      sincos_cw(e0 * s0, sa, ca);
      sincos_cw(e1 * s1, sb, cb);
      PE[n][1][4] = (_Float16)(g == 3 ? x[n][0] : sa);
      PE[n][1][5] = (_Float16)(g == 3 ? x[n][1] : ca);
      PE[n][1][6] = (_Float16)(g == 3 ? x[n][2] : sb);
      PE[n][1][7] = (_Float16)(g == 3 ? 0.0f : cb);
    }
  };
  h8 DPE[2][1];
  auto encode_dir = [&](const float (&q)[2][3]) {
    const float ds = g == 0 ? 1.0f : g == 1 ? 2.0f : g == 2 ? 4.0f : 8.0f;            // octave g
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sv, cv;
        sincos_cw(q[n][c] * ds, sv, cv);
        DPE[n][0][2 * c] = (_Float16)sv;
        DPE[n][0][2 * c + 1] = (_Float16)cv;
      }
      DPE[n][0][6] = (_Float16)(g == 0 ? q[n][0] : g == 1 ? q[n][2] : 0.0f);
      DPE[n][0][7] = (_Float16)(g == 0 ? q[n][1] : 0.0f);
    }
  };

  // software pipeline across tiles: a tile's xyz encoding is computed during the previous tile (under its views layer)
  {
    float x0[2][3];
    load_x(blockIdx.x, x0);
    encode_xyz(x0);
  }
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    h8 X[2][8], Y[2][8];
    f32x4 c = *reinterpret_cast<lds_cf32x4*>(bias_g);                           // bias of (L0, out-tile 0): one exposed LDS round trip per tile
    gemm16s_layer<2, 0, 16, 0>(r, bias_g, PE[0], PE[1], PE[0], PE[1], X[0], X[1], true, c, bias_g + 256);   // L0
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {                                            // L1..L4
      gemm16s_layer<8, 0, 16, 0>(r, bias_g + (1 + 2 * it) * 256, X[0], X[1], X[0], X[1], Y[0], Y[1], true, c, bias_g + (2 + 2 * it) * 256);
      gemm16s_layer<8, 0, 16, 0>(r, bias_g + (2 + 2 * it) * 256, Y[0], Y[1], Y[0], Y[1], X[0], X[1], true, c, bias_g + (3 + 2 * it) * 256);
    }
    gemm16s_layer<2, 8, 16, 0>(r, bias_g + 5 * 256, PE[0], PE[1], X[0], X[1], Y[0], Y[1], true, c, bias_g + 6 * 256);   // L5 = skip(PE) + hidden
    gemm16s_layer<8, 0, 16, 0>(r, bias_g + 6 * 256, Y[0], Y[1], Y[0], Y[1], X[0], X[1], true, c, bias_g + 7 * 256);      // L6
    float xn[2][3], dcur[2][3];
    load_x(tile + gridDim.x, xn);                                               // next tile's points, this tile's directions: land during L7
    if (!DENS) load_d(tile, dcur);
    gemm16s_layer<8, 0, 16, 0>(r, bias_g + 7 * 256, X[0], X[1], X[0], X[1], Y[0], Y[1], true, c, DENS ? nullptr : bias_g + 8 * 256);   // L7 -> Y = relu(h7)
    // sigma head on relu(h7): row 0 of a 16-row out-tile, 8 k-steps (fragments 0..7 of its chunk), accumulators from 0
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 sg0, sg1, unused;
    gemm16s_tile<8, 0, 0>(r, 0, Y[0], Y[1], Y[0], Y[1], zero4, sg0, sg1, nullptr, unused);
    // only row 0 is sigma: keep two scalars across the colour branch, not two accumulator quads (the compiler spilled the quads:
    // 2 KB of scratch stores per wave and tile, 7 GB of HBM writes per frame in WRITE_SIZE)
    float sig0 = sg0[0] + cst[kF16sOffHeadBias + 3], sig1 = sg1[0] + cst[kF16sOffHeadBias + 3];
    asm volatile("" : "+v"(sig0), "+v"(sig1));
    f32x4 col0 = zero4, col1 = zero4;
    bool dead_wave = false;                                                     // (wave-uniform)
    if constexpr (DSKIP) {
      const long long p0 = tile * kF16TilePts + wave * 32 + col;
      dead_wave = __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(
                      g == 0 && ((p0 < n_points && sig0 > 0.0f) || (p0 + 16 < n_points && sig1 > 0.0f))) != 0ull)) == 0;
    }
    if constexpr (DENS) {
      // density only: the stream wraps after this chunk; its other 24 fragments (the start of the feature layer) are skipped by
      // advancing the ring by hand, and the register prefetch is re-primed on the next tile's first fragments
      ring_advance(r);
#pragma unroll
      for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);
      encode_xyz(xn);
    } else if (dead_wave) {
      // (wave-uniform) no point of this wave has density: the colour branch (24 fragments of this chunk + 6 chunks) goes by unread --
      // seven chunk ends, each with this wave's DMA share and the workgroup barrier
#pragma unroll 1
      for (int cc = 0; cc < 7; ++cc) ring_advance(r);
#pragma unroll
      for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);
      encode_xyz(xn);
    } else {
      gemm16s_layer<8, 0, 16, 8>(r, bias_g + 8 * 256, Y[0], Y[1], Y[0], Y[1], X[0], X[1], false, c, bias_views_g);   // feature (no ReLU)
      h8 V[2][4];
      __builtin_amdgcn_sched_barrier(0);
      encode_dir(dcur);
      encode_xyz(xn);                 // next tile's encoding: here only X (the feature vector) is live
      gemm16s_layer<8, 1, 8, 8>(r, bias_views_g, X[0], X[1], DPE[0], DPE[1], V[0], V[1], true, c, nullptr);           // views: [feature, dirs] -> 128
      gemm16s_tile<4, 0, 16>(r, 0, V[0], V[1], V[0], V[1], zero4, col0, col1, nullptr, unused);                       // rgb head: rows 0..2, fragments 16..19
      // the 12 pad fragments behind the rgb head are never read: the chunk ends here
      ring_advance(r);
#pragma unroll
      for (int i = 0; i < kPfDist; ++i) r.pf[i] = frag_read(r, i);
    }

    if (g == 0) {
      const bool no_colour = DENS || dead_wave;                                 // (a skipped colour branch must give rgb = 0, not the bias)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const long long pl = tile * kF16TilePts + wave * 32 + 16 * n + col;
        if (pl < n_points) {
          const long long p = a.index ? (long long)a.index[pl] : pl;
          const f32x4 cc = n ? col1 : col0;
          f32x4 out;
          out.x = no_colour ? 0.0f : cc[0] + cst[kF16sOffHeadBias + 0];
          out.y = no_colour ? 0.0f : cc[1] + cst[kF16sOffHeadBias + 1];
          out.z = no_colour ? 0.0f : cc[2] + cst[kF16sOffHeadBias + 2];
          out.w = n ? sig1 : sig0;
          reinterpret_cast<f32x4*>(a.raw)[p] = out;
        }
      }
    }
  }
  // no LDS-DMA may still be in flight when the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
