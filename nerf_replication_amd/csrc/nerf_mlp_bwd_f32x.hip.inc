// Backward (data-gradient) chain of the NeRF MLP on the fp16 matrix cores with split (hi + 2^-11 lo)
// operands: the f32x counterpart of nerf_mlp_bwd_f32.hip.inc (same math, same saved tensors, same
// outputs), structured like nerf_mlp_f32x.hip.inc (LDS-DMA ring of (hi, lo) fragment pairs, m-outer
// out-tiles, gradients as packed register-resident B fragments).
// (needs nerf_mlp_f32x.hip.inc ahead of it: XRing, the training layer skeleton, XRowStage)
//
// Stream (nerf_pack_f16_kernel<bwd>): transposed weights, A fragment of (in-feature tile m, k-step s over
// the layer's OUTPUT features) = W[act16_feat(s, j, lane>>5)][32 m + (lane&31)], consumption order
//   Wv[:, :256]^T | Wf^T | W7^T | W6^T | W5[:,63:]^T | W5[:, :63]^T (PE slots) | W4^T .. W1^T | W0^T (PE slots);
// const region: w_alpha and w_rgb in accumulator-row layout (fp32).

constexpr int kXbOffWAlpha = 0;        // floats in the const region: [2][128]
constexpr int kXbOffWRgb = 256;        // [3][2][64]

// Dynamic range.  Gradients are not O(1) like activations: with a mean-reduced loss they sit around 1e-6,
// far below the smallest normal fp16 (6.1e-5), so the hi/lo split would keep only a few bits.  The chain
// is linear in the incoming gradient, so every point carries a power-of-two scale: the incoming d(loss)/d(raw)
// is normalised to max 1, each layer's output is renormalised with the maximum seen one layer earlier (exact:
// powers of two), and everything that leaves the kernel is multiplied by the inverse.
struct XbScale {
  float inv;      // 1 / (scale carried by the current B fragments)
  float adj;      // power of two applied to this layer's outputs before they are split
  float mx;       // running max |output * adj| of this layer (this lane)
};
__device__ __forceinline__ float pow2_recip(float m) {      // 2^-floor(log2 m), clamped to normal numbers
  unsigned e = (__float_as_uint(m) >> 23) & 0xffu;
  e = e < 2u ? 2u : (e > 252u ? 252u : e);
  return __uint_as_float((254u - e) << 23);
}
__device__ __forceinline__ void xb_next_layer(XbScale& sc) {
  sc.inv = sc.inv / sc.adj;                                   // exact (powers of two)
  const float m = fmaxf(sc.mx, __shfl_xor(sc.mx, 32));
  sc.adj = m > 0.0f ? pow2_recip(m) : 1.0f;
  const float ninv = sc.inv / sc.adj;                         // keep the cumulative scale far from the fp32 limits
  if (!(ninv > 0x1p-90f && ninv < 0x1p90f)) sc.adj = 1.0f;
  sc.mx = 0.0f;
}

// split a finished fp32 tile (times sc.adj) into the two packed B fragments (k-steps 2m, 2m+1) of the next GEMM
__device__ __forceinline__ void splitx_tile(const f32x16& v, int m, h8* OUTh, h8* OUTl, XbScale& sc) {
  h8 h0, h1, l0, l1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 th, tl;
    const float a = v[j] * sc.adj, b = v[8 + j] * sc.adj;
    sc.mx = fmaxf(sc.mx, fmaxf(fabsf(a), fabsf(b)));
    split16(a, th, tl); h0[j] = th; l0[j] = tl;
    split16(b, th, tl); h1[j] = th; l1[j] = tl;
  }
  OUTh[2 * m] = h0; OUTh[2 * m + 1] = h1;
  OUTl[2 * m] = l0; OUTl[2 * m + 1] = l1;
}

// Full layer: NM in-feature tiles of  g_in = W^T g_out  on the training layer skeleton (gemmx_layer_train in nerf_mlp_f32x.hip.inc:
// a finished tile is combined, masked, stored and split in eight 2-value chunks behind the MFMAs of the NEXT tile).
// EXTRA: + w_alpha * g_sigma (joins at z7).  MASK: ReLU mask from the sign bits the SAVE forward collected (TrainSave::off_bits:
// ONE coalesced 16-byte load per lane and layer -- round 2 re-read the 1-KiB activation row of every point, 8.4 GB per step).
// STORE: row-major g_z (times the inverse scale) for the weight-gradient kernels, through the per-wave LDS transpose (XRowStage in
// nerf_mlp_f32x.hip.inc: full 128-byte lines per store instead of 64 scattered 16-byte pieces -- without its stores this kernel
// was 48 % faster) -- UNCONDITIONAL: the lanes of a ragged last tile write their duplicate rows into the pad32 padding of the
// TrainGrad regions, a wave without a tile never gets here.  `tile_rows`: wave-uniform address of the tile's (row 0, feature 0).
#ifndef NERF_XB_HACK_NOSTORE
#define NERF_XB_HACK_NOSTORE 0          // timing only: the chain without its g_z row stores
#endif
template <bool EXTRA, bool MASK, bool STORE, int MM, int Q>
__device__ __forceinline__ void xb_epilogue_chunk(XPending& t, h8* OUTh, h8* OUTl, const u32x4& mw, const XRowStage& st,
                                                  lds_cfloat* extra_w, float extra_g, float (&keep)[2], float sc_inv, float sc_adj, float& sc_mx) {
  // (scalar fp32 instructions on purpose: xsplit_pair in nerf_mlp_f32x.hip.inc)
  f32x2 v;
  v.x = fmaf(t.al[2 * Q], kXLoInv, t.ah[2 * Q]); v.y = fmaf(t.al[2 * Q + 1], kXLoInv, t.ah[2 * Q + 1]);
  if constexpr (EXTRA) {
    const f32x2 w = *reinterpret_cast<lds_cf32x2*>(extra_w + MM * 16 + 2 * Q);
    v.x = fmaf(w.x, extra_g, v.x); v.y = fmaf(w.y, extra_g, v.y);
  }
  if constexpr (MASK) {
    const int w = (int)mw[MM >> 1];
    // (v_bfe_i32 by asm: hipcc turns `x & sbfe(w, pos, 1)` into and + compare + select, three VALU per value instead of two)
    int m0, m1;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m0) : "v"(w), "n"(16 * (MM & 1) + 2 * Q));
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m1) : "v"(w), "n"(16 * (MM & 1) + 2 * Q + 1));
    v.x = __int_as_float(__float_as_int(v.x) & m0);
    v.y = __int_as_float(__float_as_int(v.y) & m1);
  }
  if constexpr (STORE) {
    f32x2 o; o.x = v.x * sc_inv; o.y = v.y * sc_inv;
    if (Q & 1) {
      f32x4 o4; o4.x = keep[0]; o4.y = keep[1]; o4.z = o.x; o4.w = o.y;
      if (!NERF_XB_HACK_NOSTORE) xstage_put<(Q >> 1)>(st, o4);
    } else { keep[0] = o.x; keep[1] = o.y; }
  }
  // split (times sc.adj) into the packed B fragments (k-steps 2 MM, 2 MM + 1) of the next GEMM: same roundings as split16
  const float a0 = v.x * sc_adj, a1 = v.y * sc_adj;
  sc_mx = fmaxf(sc_mx, fmaxf(fabsf(a0), fabsf(a1)));
  h2 hi, lo;
  xsplit_pair(a0, a1, hi, lo);
  xpending_emit(t, MM, Q, hi, lo, OUTh, OUTl);
}

template <int KS, int NM, bool EXTRA, bool MASK, bool STORE>
__device__ __forceinline__ void gemmxb_layer(XRing& r, const h8* Bh, const h8* Bl, h8* OUTh, h8* OUTl,
                                             const u32x4& mw, const XRowStage& st, float* tile_rows,
                                             lds_cfloat* extra_w, float extra_g, XbScale& sc) {
  const float sc_inv = sc.inv, sc_adj = sc.adj;            // (scalars: the struct, reached through the nested lambdas, ended up in
  float sc_mx = sc.mx;                                     //  LDS-promoted stack memory -- a ds_read + vmcnt(0) drain per chunk)
  float keep[2] = {0.0f, 0.0f};
  gemmx_layer_train<KS, 0, NM, 0, 1024, STORE && !NERF_XB_HACK_NOSTORE>(r, Bh, Bl, Bh, Bl, st, tile_rows,
    [&](XPending& cur, auto) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { cur.ah[i] = 0.0f; cur.al[i] = 0.0f; }
    },
    [&](XPending& t, auto MM, auto Q) {
      xb_epilogue_chunk<EXTRA, MASK, STORE, decltype(MM)::value, decltype(Q)::value>(t, OUTh, OUTl, mw, st, extra_w, extra_g, keep, sc_inv, sc_adj, sc_mx);
    });
  sc.mx = sc_mx;
  xb_next_layer(sc);
}

// PTS: explicit points (a.pts) and per-coordinate gradient (a.g_x), as in the fp32 chain.  DENS (BwdArgs::density_only): d loss /
// d rgb is identically zero (coarse pass of a training step) -- the chain starts at g_z7 = w_alpha * g_sigma, the stream behind
// Wv^T and Wf^T (12 of 72 chunks less), no g_zv / g_f row is written (the host skips their weight-gradient jobs).
constexpr int kXbChunkW7T = 2 * (nerf::kXbStepsWfT + 128) / nerf::kF16ChunkFrags;     // 12
static_assert((2 * (nerf::kXbStepsWfT + 128)) % nerf::kF16ChunkFrags == 0, "W7^T starts a chunk");
template <bool PTS, bool DENS = false>
__global__ __launch_bounds__(kXThreads) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_mlp_bwd_f32x_kernel(BwdArgs a) {
  using namespace nerf;
  __shared__ __attribute__((aligned(128))) char smem_generic[kF16LdsBytes + kXWaves * kXStageBytes];     // weight ring + row-store transpose
  lds_char* smem = (lds_char*)smem_generic;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5;
  const char* packed = reinterpret_cast<const char*>(a.packed_bwd);
  const XRowStage st = xstage_init(smem + kF16LdsBytes + wave * kXStageBytes, lane);
  {
    const char* csrc = packed + wave * 4096 + lane * 16;
    lds_char* cdst = smem + wave * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void*)(csrc + i * 1024), (lds_void*)(cdst + i * 1024), 16, 0, 0);
  }
  XRing r;
  r.gsrc = packed + kF16ConstBytes + wave * (kXDmaPerWave * kF16FragBytes); r.lane_off = (unsigned)lane * 16u;
  r.ldst = smem + kF16ConstBytes + wave * (kXDmaPerWave * kF16FragBytes);
  r.ring = smem + kF16ConstBytes + lane * 16;
  r.cur_slot = 0; r.next_slot = 0; r.n_chunks = kXbChunks; r.first_chunk = DENS ? kXbChunkW7T : 0; r.next_chunk = r.first_chunk; r.dens = false;
  xring_issue(r); xring_issue(r); xring_issue(r);
  asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  xring_set_slots(r);
#pragma unroll
  for (int i = 0; i < kXPfDist; ++i) xfrag_read(r, i, r.pfh[i], r.pfl[i]);
  lds_cfloat* cst = reinterpret_cast<lds_cfloat*>(smem);

  const long long P = a.n_points;
  // live-tile list (BwdArgs::live_tiles): the four waves of a workgroup tile take four consecutive list entries (32-point
  // tiles).  A wave without a tile (past the end of the list / of a ragged last 128-point tile) lets the whole stream go by: it
  // still issues its share of the DMAs and meets the chunk barriers.  Every other wave stores unconditionally.
  const bool list = a.live_tiles != nullptr;                               // (uniform)
  const long long n_live = list ? (long long)*a.n_live : 0;
  const long long n_tiles = list ? (n_live + kXWaves - 1) / kXWaves : (P + kXTilePts - 1) / kXTilePts;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long entry = tile * kXWaves + wave;                         // (uniform)
    if (list ? entry >= n_live : entry * 32 >= TrainSave::pad32(P)) {
#pragma unroll 1
      for (int c = 0; c < kXbChunks - (DENS ? kXbChunkW7T : 0); ++c) {
#pragma unroll
        for (int i = 0; i < kXDmaPerWave; ++i) xring_issue_part(r, i);
        xring_advance(r);
      }
#pragma unroll
      for (int i = 0; i < kXPfDist; ++i) xfrag_read(r, i, r.pfh[i], r.pfl[i]);
      continue;
    }
    const long long tile32 = list ? (long long)uniform_load_i32(a.live_tiles + entry) : entry;     // this wave's 32-point tile
    const long long prow = tile32 * 32 + (lane & 31);                      // row of the TrainGrad regions (< pad32(P))
    const bool valid = prow < P;
    const long long p = valid ? prow : P - 1;
    f32x4 g = reinterpret_cast<const f32x4*>(a.draw)[p];
    if constexpr (DENS) { g.x = 0.0f; g.y = 0.0f; g.z = 0.0f; }
    const float gw_true = g.w;
    XbScale sc;
    {
      const float gm = fmaxf(fmaxf(fabsf(g.x), fabsf(g.y)), fmaxf(fabsf(g.z), fabsf(g.w)));
      const float s0 = gm > 0.0f ? pow2_recip(gm) : 1.0f;
      g.x *= s0; g.y *= s0; g.z *= s0; g.w *= s0;
      sc.inv = 1.0f / s0; sc.adj = 1.0f; sc.mx = 0.0f;
    }
    // wave-uniform address of (row 0, feature 0) of this wave's 32-point tile in a row-major TrainGrad region
    auto srow = [&](long long off, int width) -> float* { return a.gsave + off + tile32 * (32LL * width); };
    // ReLU sign bits of this wave's 32-point tile (written by the f32x SAVE forward in the fp32 forward's layout)
    auto mbits = [&](int which) -> const u32x4* {
      const char* base = reinterpret_cast<const char*>(a.save + TrainSave::off_bits(P) + TrainSave::bits_block(tile32, which));
      return reinterpret_cast<const u32x4*>(base + (unsigned)(lane * 16));
    };

    // every global load of the tile is issued HERE, in front of the layers: hipcc waits for an ordinary load's result with
    // vmcnt(0) while an LDS-DMA is in flight (always, in this kernel), i.e. each use of a freshly loaded mask in the middle of
    // the chain drained the weight ring and every row store behind it -- two full drains per layer in the round-2 kernel
    const u32x4 no_mask = {0u, 0u, 0u, 0u};
    const u32x4 mk8 = DENS ? no_mask : *mbits(8), mk7 = *mbits(7), mk6 = *mbits(6), mk5 = *mbits(5), mk4 = *mbits(4),
                mk3 = *mbits(3), mk2 = *mbits(2), mk1 = *mbits(1), mk0 = *mbits(0);       // (named: an indexed array would live in scratch)
    const long long ray = p / a.n_samples;
    float px[3];
    {
      const bool want = (PTS ? a.g_x : a.g_t) != nullptr;
      const int s_idx = (int)(p - ray * a.n_samples);
      const float t = (PTS || !want) ? 0.0f : a.tvals[ray * a.t_ray_stride + s_idx];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        px[c] = !want ? 0.0f : PTS ? a.pts[p * 3 + c] : __fadd_rn(a.rays_o[ray * 3 + c], __fmul_rn(a.rays_d[ray * 3 + c], t));
    }
    float rd[3] = {0.f, 0.f, 0.f};
    if (!PTS && a.g_t != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) rd[c] = a.rays_d[ray * 3 + c];
    }
    h8 Xh[16], Xl[16], Yh[16], Yl[16];
    if constexpr (!DENS) {
    // g_zv = (Wr^T g_rgb) * (hv > 0): tile by tile, straight into B fragments
    h8 Vh[8], Vl[8];
    {
      const u32x4 hvw = mk8;                            // sign bits of the views layer (4 tiles: words 0, 1)
      float* st_row = srow(TrainGrad::off_gzv(P), 128);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        f32x16 v;
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = 0.0f;
        const float gc[3] = {g.x, g.y, g.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          lds_cf32x4* w = reinterpret_cast<lds_cf32x4*>(cst + kXbOffWRgb + (c * 2 + h) * 64 + m * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 w4 = w[q];
            v[4 * q + 0] = fmaf(w4.x, gc[c], v[4 * q + 0]); v[4 * q + 1] = fmaf(w4.y, gc[c], v[4 * q + 1]);
            v[4 * q + 2] = fmaf(w4.z, gc[c], v[4 * q + 2]); v[4 * q + 3] = fmaf(w4.w, gc[c], v[4 * q + 3]);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int hw = (int)hvw[m >> 1];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[4 * q + e] = __int_as_float(__float_as_int(v[4 * q + e]) & __builtin_amdgcn_sbfe(hw, 16 * (m & 1) + 4 * q + e, 1));
          f32x4 o4; o4.x = v[4 * q + 0] * sc.inv; o4.y = v[4 * q + 1] * sc.inv; o4.z = v[4 * q + 2] * sc.inv; o4.w = v[4 * q + 3] * sc.inv;
          if (q == 0) xstage_put<0>(st, o4); else if (q == 1) xstage_put<1>(st, o4); else if (q == 2) xstage_put<2>(st, o4); else xstage_put<3>(st, o4);
        }
        xstage_flush<512>(st, st_row, m);
        splitx_tile(v, m, Vh, Vl, sc);
      }
      xb_next_layer(sc);
    }
    gemmxb_layer<8, 8, false, false, true>(r, Vh, Vl, Xh, Xl, no_mask, st, srow(TrainGrad::off_gf(P), 256), nullptr, 0.f, sc);                 // g_f
    // w_alpha * g_sigma joins at z7 with a magnitude of its own: cap the renormalisation so it cannot overflow fp16
    if (gw_true != 0.0f) sc.adj = fminf(sc.adj, pow2_recip(fabsf(gw_true)) * 0.25f * sc.inv);
    gemmxb_layer<16, 8, true, true, true>(r, Xh, Xl, Yh, Yl, mk7, st, srow(TrainGrad::off_gz(P, 7), 256), cst + kXbOffWAlpha + h * 128, gw_true / sc.inv, sc);  // g_z7
    } else {
      // g_z7 = (w_alpha * g_sigma) * (h7 > 0): no GEMM in front of it (g_f = 0)
      const u32x4 mw = mk7;
      float* st_row = srow(TrainGrad::off_gz(P, 7), 256);
      lds_cfloat* wa = cst + kXbOffWAlpha + h * 128;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        f32x16 v;
        const int w = (int)mw[m >> 1];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w4 = reinterpret_cast<lds_cf32x4*>(wa + m * 16)[q];
          const float wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[4 * q + e] = __int_as_float(__float_as_int(wq[e] * g.w) & __builtin_amdgcn_sbfe(w, 16 * (m & 1) + 4 * q + e, 1));
          f32x4 o4; o4.x = v[4 * q + 0] * sc.inv; o4.y = v[4 * q + 1] * sc.inv; o4.z = v[4 * q + 2] * sc.inv; o4.w = v[4 * q + 3] * sc.inv;
          if (q == 0) xstage_put<0>(st, o4); else if (q == 1) xstage_put<1>(st, o4); else if (q == 2) xstage_put<2>(st, o4); else xstage_put<3>(st, o4);
        }
        xstage_flush<1024>(st, st_row, m);
        splitx_tile(v, m, Yh, Yl, sc);
      }
      xb_next_layer(sc);
    }
    gemmxb_layer<16, 8, false, true, true>(r, Yh, Yl, Xh, Xl, mk6, st, srow(TrainGrad::off_gz(P, 6), 256), nullptr, 0.f, sc);                // g_z6
    gemmxb_layer<16, 8, false, true, true>(r, Xh, Xl, Yh, Yl, mk5, st, srow(TrainGrad::off_gz(P, 5), 256), nullptr, 0.f, sc);                // g_z5
    const float inv_z5 = sc.inv;                                       // scale of the g_z5 fragments (Y), used again below
    gemmxb_layer<16, 8, false, true, true>(r, Yh, Yl, Xh, Xl, mk4, st, srow(TrainGrad::off_gz(P, 4), 256), nullptr, 0.f, sc);                // g_z4 (W5[:,63:]^T)
    // the two PE-slot GEMMs (W5[:, :63]^T g_z5 and W0^T g_z0) are contracted with d(PE)/dx straight away, so
    // only three partial sums per lane stay live across the layers in between
    float gx[3] = {0.f, 0.f, 0.f};
    auto pe_contract = [&](const f32x16& G0, const f32x16& G1, float inv) {
      if ((PTS ? a.g_x : a.g_t) == nullptr) return;
      const float hs = h ? 32.0f : 1.0f;
#pragma unroll
      for (int ai = 0; ai < 15; ++ai) {
        const int c = ai % 3;
        const float x = px[c];
        const float f = hs * (float)(1 << (ai / 3));
        float sv, cv;
        sincos_cw(x * f, sv, cv);
        const int n0 = 2 * ai, n1 = 2 * ai + 1;
        gx[c] += f * inv * (cv * (n0 < 16 ? G0[n0 & 15] : G1[n0 & 15]) - sv * (n1 < 16 ? G0[n1 & 15] : G1[n1 & 15]));
      }
      if (h) gx[2] += inv * G1[14]; else { gx[0] += inv * G1[14]; gx[1] += inv * G1[15]; }
    };
    {
      const f32x16 t0 = gemmx_tile<16, 0, 0, false>(r, Yh, Yl, Yh, Yl), t1 = gemmx_tile<16, 0, 0, false>(r, Yh, Yl, Yh, Yl);    // W5[:, :63]^T g_z5
      pe_contract(t0, t1, inv_z5);
    }
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
      gemmxb_layer<16, 8, false, true, true>(r, Xh, Xl, Yh, Yl, (it ? mk1 : mk3), st, srow(TrainGrad::off_gz(P, 3 - 2 * it), 256), nullptr, 0.f, sc);   // g_z3, g_z1
      gemmxb_layer<16, 8, false, true, true>(r, Yh, Yl, Xh, Xl, (it ? mk0 : mk2), st, srow(TrainGrad::off_gz(P, 2 - 2 * it), 256), nullptr, 0.f, sc);   // g_z2, g_z0
    }
    {
      const f32x16 t0 = gemmx_tile<16, 0, 0, false>(r, Xh, Xl, Xh, Xl), t1 = gemmx_tile<16, 0, 0, false>(r, Xh, Xl, Xh, Xl);    // W0^T g_z0
      pe_contract(t0, t1, sc.inv);
    }
    if (PTS) {
      if (a.g_x != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float gc = gx[c] + __shfl_xor(gx[c], 32);
          if (valid && h == 0) a.g_x[p * 3 + c] = gc;
        }
      }
    } else if (a.g_t != nullptr) {
      uintptr_t out = reinterpret_cast<uintptr_t>(a.g_t);
      // (opaque here: hoisted out of the tile loop, the decoded g_x address was one more SGPR pair live across the chain, and the
      //  density instance spilled to scratch)
      asm volatile("" : "+s"(out));
      if (out & 1) {                                    // g_x (see BwdArgs::g_t)
        float* const gxp = reinterpret_cast<float*>(out - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float gc = gx[c] + __shfl_xor(gx[c], 32);
          if (valid && h == 0) gxp[p * 3 + c] = gc;
        }
      } else {
        float gt = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) gt += (gx[c] + __shfl_xor(gx[c], 32)) * rd[c];
        if (valid && h == 0) reinterpret_cast<float*>(out)[p] = gt;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
