// Multiresolution hash-grid encoding (instant-NGP): forward, embedding gradient, input gradient (DESIGN.md section 2.12).
// fp32 throughout; the unit is compiled with -ffp-contract=off, so every multiply and add below rounds on its own and the forward
// is bit for bit the fixed-order fp32 restatement in tests/hashgrid_reference.py.
//
// A level is a table of n = offsets[l+1] - offsets[l] rows of C floats.  A point x in [0,1]^D sits in the cell
//     pos_d = x_d * scale + 0.5,  g_d = floor(pos_d),  f_d = pos_d - g_d                       (scale: host float, one per level)
// and mixes the 2^D corners g + bit_d(idx) with the weights prod_d (bit_d ? f_d : 1 - f_d).  The row of a corner, all in uint32 with
// wrap-around: with stride = 1 and, for d = 0..D-1 while stride <= n, index += g_d * stride, stride *= resolution + 1; if the stride
// ends above n the index is instead the XOR of g_d * prime_d; the row is index mod n.  Whether a level is dense or hashed, and its
// strides, depend on (n, resolution) alone: HgLevel works them out once per thread (wave-uniform, scalar registers) and a corner costs
// D multiplies, D adds or XORs and the modulo.  Every row is reduced modulo n, so no input, finite or not, reaches outside its level.
//
// Lane mappings:
//   forward          one thread per point, one level per blockIdx.y (one level's table is what the caches hold at a time); a row is one
//                    4*C-byte vector load, the C results one vector store into out[b, l*C ..] -- the output is [B, L*C] as it stands.
//   embedding grad   one thread per (point, channel), channel fastest, one level per blockIdx.y: the C adds into one row sit on C
//                    neighbouring lanes, so a wave-instruction carries 64/C row segments of 4*C contiguous bytes and every row costs
//                    ONE memory-side atomic request.  (One lane per row with C adds of its own would put 64 rows into each of C
//                    instructions: C requests per row, the "one lane per row" shape that runs an order of magnitude under the
//                    contiguous rate.)  No-return global fp32 atomic adds into a buffer the caller zeroed: the entry accumulates.
//   input grad       one thread per point, levels in a loop; the 2^D corner rows are loaded once per level and serve all D axes;
//                    nothing is stored in the forward.  grad_x is written, not accumulated; no atomics.
#include "nerf_host.h"

namespace {

constexpr int kHgBlock = 256;
constexpr int kHgMaxLevels = 32;

struct HgLevels {                              // passed by value in the kernel arguments: no device allocation
  int offsets[kHgMaxLevels + 1];
  float scales[kHgMaxLevels];
};

template <int C> struct HgRow;
template <> struct HgRow<1> { typedef float type; };
template <> struct HgRow<2> { typedef float2 type; };
template <> struct HgRow<4> { typedef float4 type; };

// one row of C floats (4*C-byte aligned: the entries check it) -> v[C]
template <int C>
__device__ __forceinline__ void hg_load_row(const float* __restrict__ p, float (&v)[C]) {
  if constexpr (C == 8) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    typedef typename HgRow<C>::type R;
    const R r = *reinterpret_cast<const R*>(p);
    __builtin_memcpy(v, &r, sizeof(R));
  }
}
template <int C>
__device__ __forceinline__ void hg_store_row(float* __restrict__ p, const float (&v)[C]) {
  if constexpr (C == 8) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    typedef typename HgRow<C>::type R;
    R r;
    __builtin_memcpy(&r, v, sizeof(R));
    *reinterpret_cast<R*>(p) = r;
  }
}

// float -> uint32 with the out-of-range cases defined (negative and NaN -> 0, huge -> 2^32 - 256); in [0, 2^32) it is the plain cast
__device__ __forceinline__ uint32_t hg_to_u32(float v) { return (uint32_t)fminf(fmaxf(v, 0.0f), 4294967040.0f); }

template <int D>
struct HgLevel {
  uint32_t n;            // rows of the level (> 0: the entries check it)
  uint32_t mul[D];       // dense: the (wrapped) stride of axis d; hashed: its prime
  bool hashed;
  bool pow2;
  float scale;
  __device__ __forceinline__ HgLevel(const HgLevels& lv, int l) {
    const uint32_t primes[4] = {1u, 19349663u, 83492791u, 25165843u};
    n = (uint32_t)(lv.offsets[l + 1] - lv.offsets[l]);
    scale = lv.scales[l];
    const uint32_t res1 = hg_to_u32(ceilf(scale)) + 2u;       // resolution + 1, resolution = uint32(ceil(scale)) + 1
    uint32_t stride = 1;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      mul[d] = stride;
      if (stride <= n) stride *= res1;                        // (once above n it stays there: the walk has ended)
    }
    hashed = stride > n;
    if (hashed) {
#pragma unroll
      for (int d = 0; d < D; ++d) mul[d] = primes[d];
    }
    pow2 = (n & (n - 1u)) == 0u;
  }
  __device__ __forceinline__ uint32_t row(const uint32_t (&g)[D]) const {
    uint32_t index = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const uint32_t t = g[d] * mul[d];
      index = hashed ? (index ^ t) : (index + t);
    }
    return pow2 ? (index & (n - 1u)) : (index % n);
  }
};

template <int D>
struct HgCell {
  uint32_t g[D];
  float f[D], omf[D];    // the fraction and 1 - fraction
  __device__ __forceinline__ HgCell(const float* __restrict__ x, float scale) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float pos = x[d] * scale + 0.5f;
      const float fl = floorf(pos);
      g[d] = hg_to_u32(fl);
      f[d] = pos - fl;
      omf[d] = 1.0f - f[d];
    }
  }
  // corner idx: its grid position and weight (1.0f times the factors in axis order)
  __device__ __forceinline__ float corner(int idx, uint32_t (&gc)[D]) const {
    float w = 1.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const bool hi = (idx >> d) & 1;
      gc[d] = g[d] + (hi ? 1u : 0u);
      w *= hi ? f[d] : omf[d];
    }
    return w;
  }
};

template <int D, int C>
__global__ __launch_bounds__(kHgBlock)
void nerf_hashgrid_forward_kernel(const float* __restrict__ x, const float* __restrict__ emb, uint32_t B, uint32_t L, HgLevels lv,
                                  float* __restrict__ out) {
  const uint32_t b = blockIdx.x * kHgBlock + threadIdx.x;
  if (b >= B) return;
  const int l = blockIdx.y;
  const HgLevel<D> level(lv, l);
  const HgCell<D> cell(x + b * D, level.scale);
  const float* __restrict__ table = emb + (size_t)lv.offsets[l] * C;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int idx = 0; idx < (1 << D); ++idx) {
    uint32_t gc[D];
    const float w = cell.corner(idx, gc);
    float e[C];
    hg_load_row<C>(table + (size_t)level.row(gc) * C, e);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += w * e[c];
  }
  hg_store_row<C>(out + (b * L + l) * C, acc);                // B*L*C < 2^31: the entry checks it
}

template <int D, int C>
__global__ __launch_bounds__(kHgBlock)
void nerf_hashgrid_grad_emb_kernel(const float* __restrict__ x, const float* __restrict__ grad_out, uint32_t B, uint32_t L,
                                   HgLevels lv, float* __restrict__ grad_emb) {
  const uint32_t t = blockIdx.x * kHgBlock + threadIdx.x;     // B*C < 2^31
  const uint32_t b = t / C, c = t % C;
  if (b >= B) return;
  const int l = blockIdx.y;
  const HgLevel<D> level(lv, l);
  const HgCell<D> cell(x + b * D, level.scale);
  const float go = grad_out[(b * L + l) * C + c];
  float* __restrict__ table = grad_emb + (size_t)lv.offsets[l] * C + c;
#pragma unroll
  for (int idx = 0; idx < (1 << D); ++idx) {
    uint32_t gc[D];
    const float w = cell.corner(idx, gc);
    atomicAdd(table + (size_t)level.row(gc) * C, w * go);     // result unused: the no-return form
  }
}

template <int D, int C>
__global__ __launch_bounds__(kHgBlock)
void nerf_hashgrid_grad_x_kernel(const float* __restrict__ x, const float* __restrict__ emb, const float* __restrict__ grad_out,
                                 uint32_t B, uint32_t L, HgLevels lv, float* __restrict__ grad_x) {
  const uint32_t b = blockIdx.x * kHgBlock + threadIdx.x;
  if (b >= B) return;
  float xs[D], gx[D];
#pragma unroll
  for (int d = 0; d < D; ++d) { xs[d] = x[b * D + d]; gx[d] = 0.0f; }
  for (uint32_t l = 0; l < L; ++l) {
    const HgLevel<D> level(lv, (int)l);
    const HgCell<D> cell(xs, level.scale);
    const float* __restrict__ table = emb + (size_t)lv.offsets[l] * C;
    float e[1 << D][C];
#pragma unroll
    for (int idx = 0; idx < (1 << D); ++idx) {
      uint32_t gc[D];
      cell.corner(idx, gc);
      hg_load_row<C>(table + (size_t)level.row(gc) * C, e[idx]);
    }
    float go[C];
    hg_load_row<C>(grad_out + (b * L + l) * C, go);
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
      for (int idx = 0; idx < (1 << D); ++idx) {
        if ((idx >> d) & 1) continue;                         // idx: the left corner (bit d clear); idx | 1 << d: the right one
        float w = level.scale;
#pragma unroll
        for (int a = 0; a < D; ++a)
          if (a != d) w *= ((idx >> a) & 1) ? cell.f[a] : cell.omf[a];
#pragma unroll
        for (int c = 0; c < C; ++c) gx[d] += go[c] * (w * (e[idx | (1 << d)][c] - e[idx][c]));
      }
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) grad_x[b * D + d] = gx[d];
}

template <int N> struct HgInt { static constexpr int value = N; };

// f(HgInt<D>, HgInt<C>) for the built pairs; the caller has checked D and C
template <class F>
int hg_dispatch(int D, int C, F&& f) {
#define NERF_HG_CASE(d, c) case (d) * 16 + (c): return f(HgInt<d>(), HgInt<c>());
  switch (D * 16 + C) {
    NERF_HG_CASE(2, 1) NERF_HG_CASE(2, 2) NERF_HG_CASE(2, 4) NERF_HG_CASE(2, 8)
    NERF_HG_CASE(3, 1) NERF_HG_CASE(3, 2) NERF_HG_CASE(3, 4) NERF_HG_CASE(3, 8)
    NERF_HG_CASE(4, 1) NERF_HG_CASE(4, 2) NERF_HG_CASE(4, 4) NERF_HG_CASE(4, 8)
  }
#undef NERF_HG_CASE
  return NERF_ERR_UNSUPPORTED;
}

bool hg_aligned(const void* p, int C) { return ((uintptr_t)p & (uintptr_t)(4 * C - 1)) == 0; }

// everything both entries check before a launch; fills `lv`
int hg_check(const char* entry, int64_t B, int32_t D, int32_t C, int32_t L, const int32_t* offsets_host, const float* scales_host,
             HgLevels& lv) {
  if (D < 2 || D > 4) return fail(NERF_ERR_UNSUPPORTED, "%s: input_dim must be 2, 3 or 4", entry);
  if (C != 1 && C != 2 && C != 4 && C != 8) return fail(NERF_ERR_UNSUPPORTED, "%s: level_dim must be 1, 2, 4 or 8", entry);
  if (L < 1 || L > kHgMaxLevels) return fail(NERF_ERR_UNSUPPORTED, "%s: num_levels must be 1..32", entry);
  if (B <= 0) return fail(NERF_ERR_INVALID_ARG, "%s: the batch must be positive", entry);
  // the kernels index x, out and grad_out with 32 bits
  if (B > 0x7fffffffLL / ((int64_t)L * C) || B > 0x7fffffffLL / D)
    return fail(NERF_ERR_INVALID_ARG, "%s: B*L*C (or B*D) exceeds 2^31 - 1: encode in chunks", entry);
  if (!offsets_host || !scales_host) return fail(NERF_ERR_INVALID_ARG, "%s: null level table", entry);
  if (offsets_host[0] < 0) return fail(NERF_ERR_INVALID_ARG, "%s: negative offset", entry);
  for (int l = 0; l < L; ++l) {
    if (offsets_host[l + 1] <= offsets_host[l]) return fail(NERF_ERR_INVALID_ARG, "%s: offsets must increase (a level needs rows)", entry);
    lv.offsets[l] = offsets_host[l];
    lv.scales[l] = scales_host[l];
  }
  lv.offsets[L] = offsets_host[L];
  for (int l = L; l < kHgMaxLevels; ++l) { lv.offsets[l + 1] = offsets_host[L]; lv.scales[l] = 0.0f; }
  return NERF_OK;
}

inline dim3 hg_grid(int64_t threads, int L) { return dim3((unsigned)((threads + kHgBlock - 1) / kHgBlock), (unsigned)L); }

}  // namespace

extern "C" {

int32_t nerf_hashgrid_forward(const float* x, const float* emb, int64_t B, int32_t D, int32_t C, int32_t L,
                              const int32_t* offsets_host, const float* scales_host, float* out, void* stream) {
  HgLevels lv;
  int rc = hg_check("nerf_hashgrid_forward", B, D, C, L, offsets_host, scales_host, lv);
  if (rc) return rc;
  if (!x || !emb || !out) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_hashgrid_forward: null argument");
  if (!hg_aligned(emb, C) || !hg_aligned(out, C))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_hashgrid_forward: emb and out must be aligned to 4*C bytes");
  return hg_dispatch(D, C, [&](auto d, auto c) {
    return NERF_LAUNCH((nerf_hashgrid_forward_kernel<decltype(d)::value, decltype(c)::value>), hg_grid(B, L), dim3(kHgBlock),
                       (hipStream_t)stream, x, emb, (uint32_t)B, (uint32_t)L, lv, out);
  });
}

int32_t nerf_hashgrid_backward(const float* x, const float* emb, const float* grad_out, int64_t B, int32_t D, int32_t C, int32_t L,
                               const int32_t* offsets_host, const float* scales_host, float* grad_emb, float* grad_x, void* stream) {
  HgLevels lv;
  int rc = hg_check("nerf_hashgrid_backward", B, D, C, L, offsets_host, scales_host, lv);
  if (rc) return rc;
  if (!x || !grad_out || (grad_x && !emb)) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_hashgrid_backward: null argument");
  if (!hg_aligned(grad_out, C) || (grad_x && !hg_aligned(emb, C)))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_hashgrid_backward: emb and grad_out must be aligned to 4*C bytes");
  hipStream_t st = (hipStream_t)stream;
  if (grad_emb) {
    rc = hg_dispatch(D, C, [&](auto d, auto c) {
      return NERF_LAUNCH((nerf_hashgrid_grad_emb_kernel<decltype(d)::value, decltype(c)::value>), hg_grid(B * C, L), dim3(kHgBlock),
                         st, x, grad_out, (uint32_t)B, (uint32_t)L, lv, grad_emb);
    });
    if (rc) return rc;
  }
  if (grad_x) {
    rc = hg_dispatch(D, C, [&](auto d, auto c) {
      return NERF_LAUNCH((nerf_hashgrid_grad_x_kernel<decltype(d)::value, decltype(c)::value>), hg_grid(B, 1), dim3(kHgBlock), st, x,
                         emb, grad_out, (uint32_t)B, (uint32_t)L, lv, grad_x);
    });
  }
  return rc;
}

}  // extern "C"
