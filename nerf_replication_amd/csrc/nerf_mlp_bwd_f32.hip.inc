// Backward (data-gradient) chain of the NeRF MLP, exact fp32 on v_mfma_f32_32x32x2_f32.
// (needs nerf_mlp_f32.hip.inc ahead of it: the weight ring, gemm_tiles and the taps)
//
// What autograd does for NeRF.forward (network.py:49-74) between grad(raw [P,4]) and
// grad(z_l) of every layer, plus grad(points) through the positional encoding (freq.py:31-32):
//   g_hv = Wr^T g_rgb;  g_zv = g_hv * (hv>0);  g_f = Wv[:, :256]^T g_zv;
//   g_h7 = Wf^T g_f + w_alpha g_sigma;  g_z7 = g_h7 * (h7>0);  g_h6 = W7^T g_z7; ... ;
//   g_h4 = W5[:, 63:]^T g_z5,  g_pe = W5[:, :63]^T g_z5 + W0^T g_z0;  g_x = (d pe / d x)^T g_pe.
// Same structure as the forward kernel: one wave owns 32 points, the gradient lives in MFMA
// accumulator layout and is fed unchanged as the next (previous) layer's B operand; only the weight
// stream differs (transposed, nerf_pack_bwd_kernel).  ReLU masks come from the activations the
// SAVE-mode forward stored; every g_z is stored row-major for the weight-gradient GEMMs.

// acc *= (activation > 0) from the sign bits the SAVE forward collected (TrainSave::off_bits): bit 16*(t&1) + r of word
// t>>1 belongs to register r of tile t.  v_bfe_i32 turns the bit into 0 / ~0, v_and applies it: two VALU per value,
// and the whole layer's mask is one 16-byte load per lane, fetched a layer ahead.
template <int NT>
__device__ __forceinline__ void mask_bits(f32x16 (&A)[NT], const u32x4& m) {
  if (NERF_BWD_HACK_NOMASK) return;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int w = (int)m[t >> 1];
#pragma unroll
    for (int r = 0; r < 16; ++r)
      A[t][r] = __int_as_float(__float_as_int(A[t][r]) & __builtin_amdgcn_sbfe(w, 16 * (t & 1) + r, 1));
  }
}

template <int NT>
__device__ __forceinline__ void zero_tiles(f32x16 (&A)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) A[t][r] = 0.0f;
}

template <bool PTS>           // PTS: points given explicitly (a.pts), gradient returned per coordinate (a.g_x)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_mlp_bwd_f32_kernel(BwdArgs a) {
  using namespace nerf;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
  long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (a.live_tiles != nullptr) {                     // (uniform) before anything is in flight: dead tiles have no slot at all
    if (tile >= *a.n_live) return;
    tile = uniform_load_i32(a.live_tiles + tile);
  }
  const long long base = tile * kTilePts;
  if (base >= a.n_points) return;
  const long long P = a.n_points;
  const long long pl = base + (lane & 31);
  const bool valid = pl < P;
  const long long p = valid ? pl : P - 1;          // clamped lanes recompute the last point and store nothing

  const float* __restrict__ pk = a.packed_bwd;
  // the weight ring in asm-load form like the forward kernels: possible since the chain no longer spills (the ReLU
  // masks come as sign bits, the rows go out through the taps); tools/check_asm_stream.py covers these instances too
  AStream ws;
  const bool dens = a.density_only != 0;                             // (uniform)
  wstream_start(ws, reinterpret_cast<const f32x4*>(pk + (dens ? kBwdOffW7T : 0)), lane);

  const f32x4 g = reinterpret_cast<const f32x4*>(a.draw)[p];      // (g_r, g_g, g_b, g_sigma)
  // ReLU masks: one 16-byte load per lane and layer from the sign-bit blocks of the SAVE forward, a layer ahead
  const u32x4* mbits = reinterpret_cast<const u32x4*>(a.save + TrainSave::off_bits(P) + TrainSave::bits_block(base / kTilePts, 0)) + lane;
  auto mask_of = [&](int which) { return mbits[which * 64]; };
  u32x4 m_cur = mask_of(8), m_next = mask_of(7);
  // every g_z row is stored by the GEMM that consumes it (tap: one 16-byte store per 4-k-step group); idle lanes of a
  // ragged last tile write the padding rows of the region (TrainGrad is pad32-sized), so no store is predicated
  float* const grow = a.gsave + pl * 256 + 4 * h;                   // + region offset (256-wide rows)

  // g_zv = (Wr^T g_rgb) * (hv > 0)
  f32x16 X[8], Y[8];
  if (!dens) {
  f32x16 V[4];
  {
    const float gc[3] = {g.x, g.y, g.z};
    zero_tiles<4>(V);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4* wr = reinterpret_cast<const f32x4*>(pk + kBwdOffWRgb + (c * 2 + h) * 64);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w4 = wr[t * 4 + q];
          V[t][4 * q + 0] = fmaf(w4.x, gc[c], V[t][4 * q + 0]);
          V[t][4 * q + 1] = fmaf(w4.y, gc[c], V[t][4 * q + 1]);
          V[t][4 * q + 2] = fmaf(w4.z, gc[c], V[t][4 * q + 2]);
          V[t][4 * q + 3] = fmaf(w4.w, gc[c], V[t][4 * q + 3]);
        }
    }
    mask_bits<4>(V, m_cur);
  }
  zero_tiles<8>(X);
  gemm_tiles<4, 8, false>(X, V, ws, StoreTap<true>{a.gsave + TrainGrad::off_gzv(P) + pl * 128 + 4 * h, nullptr});   // g_f = Wv[:, :256]^T g_zv
  }

  // The two PE-slot GEMMs (W5[:, :63]^T g_z5 and W0^T g_z0) are contracted with d(PE)/dx as soon as they exist, so
  // three partial sums per lane stay live across the layers in between instead of two accumulator tiles
  // (keeping them cost 121 spilled VGPRs).
  const long long ray = p / a.n_samples;
  float gx[3] = {0.f, 0.f, 0.f};
  auto pe_contract = [&](const f32x16 (&G)[2]) {
    if ((PTS ? a.g_x : a.g_t) == nullptr) return;
    // g_x = (d pe / d x)^T g_pe: slot 2ai = sin(2^k x_c) -> 2^k cos, slot 2ai+1 = cos -> -2^k sin; 30,31 raw
    const int s_idx = (int)(p - ray * a.n_samples);
    const float t = PTS ? 0.0f : a.tvals[ray * a.t_ray_stride + s_idx];
    const float hs = h ? 32.0f : 1.0f;
#pragma unroll
    for (int ai = 0; ai < 15; ++ai) {
      const int c = ai % 3;
      const float x = PTS ? a.pts[p * 3 + c] : __fadd_rn(a.rays_o[ray * 3 + c], __fmul_rn(a.rays_d[ray * 3 + c], t));
      const float f = hs * (float)(1 << (ai / 3));
      float sv, cv;
      sincos_cw(x * f, sv, cv);                // 1e-7 abs: plenty for a gradient, and no slow path to spill around
      const int n0 = 2 * ai, n1 = 2 * ai + 1;
      gx[c] += f * (cv * G[n0 >> 4][n0 & 15] - sv * G[n1 >> 4][n1 & 15]);
    }
    if (h) gx[2] += G[1][14]; else { gx[0] += G[1][14]; gx[1] += G[1][15]; }
  };
#pragma unroll 1
  for (int pr = 0; pr < 4; ++pr) {
    // X -> Y : Wf^T (-> g_h7), W6^T (-> g_h5), W4^T (-> g_h3), W2^T (-> g_h1); X = g_f, then g_z6, g_z4, g_z2: stored here
    zero_tiles<8>(Y);
    if (!(dens && pr == 0))          // (density only: g_f = 0, so g_h7 is just the alpha term below)
      gemm_tiles<8, 8, false>(Y, X, ws, StoreTap<true>{grow + (pr == 0 ? TrainGrad::off_gf(P) : TrainGrad::off_gz(P, 8 - 2 * pr)), nullptr});
    if (pr == 0) {                                   // + w_alpha * g_sigma (alpha_linear acts on h7 too)
      const f32x4* wa = reinterpret_cast<const f32x4*>(pk + kBwdOffWAlpha + h * 128);
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w4 = wa[t * 4 + q];
          Y[t][4 * q + 0] = fmaf(w4.x, g.w, Y[t][4 * q + 0]);
          Y[t][4 * q + 1] = fmaf(w4.y, g.w, Y[t][4 * q + 1]);
          Y[t][4 * q + 2] = fmaf(w4.z, g.w, Y[t][4 * q + 2]);
          Y[t][4 * q + 3] = fmaf(w4.w, g.w, Y[t][4 * q + 3]);
        }
    }
    const int la = 7 - 2 * pr;                       // h7, h5, h3, h1
    m_cur = m_next; m_next = mask_of(la - 1);
    mask_bits<8>(Y, m_cur);
    // Y -> X : W7^T (-> g_h6), W5[:,63:]^T (-> g_h4), W3^T (-> g_h2), W1^T (-> g_h0); Y = g_z(la): stored here
    zero_tiles<8>(X);
    gemm_tiles<8, 8, false>(X, Y, ws, StoreTap<true>{grow + TrainGrad::off_gz(P, la), nullptr});
    const int lb = 6 - 2 * pr;                       // h6, h4, h2, h0
    m_cur = m_next; m_next = mask_of(lb > 0 ? lb - 1 : 0);
    mask_bits<8>(X, m_cur);
    if (pr == 1) {                                   // skip connection: g_pe = W5[:, :63]^T g_z5
      f32x16 G5[2];
      zero_tiles<2>(G5);
      gemm_tiles<8, 2>(G5, Y, ws);
      pe_contract(G5);
    }
  }
  {
    f32x16 G0[2];
    zero_tiles<2>(G0);
    // g_pe += W0^T g_z0; X = g_z0: stored here
    gemm_tiles<8, 2, true>(G0, X, ws, StoreTap<true>{grow + TrainGrad::off_gz(P, 0), nullptr});   // last call: the asm form stops at the stream end
    pe_contract(G0);
  }

  if (PTS) {
    if (a.g_x != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float gc = gx[c] + __shfl_xor(gx[c], 32);
        if (valid && h == 0) a.g_x[p * 3 + c] = gc;
      }
    }
  } else if (reinterpret_cast<uintptr_t>(a.g_t) & 1) {       // g_x (see BwdArgs::g_t)
    float* const gxp = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(a.g_t) - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gc = gx[c] + __shfl_xor(gx[c], 32);
      if (valid && h == 0) gxp[p * 3 + c] = gc;
    }
  } else if (a.g_t != nullptr) {
    float gt = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gt += (gx[c] + __shfl_xor(gx[c], 32)) * a.rays_d[ray * 3 + c];
    if (valid && h == 0) a.g_t[p] = gt;
  }
}
