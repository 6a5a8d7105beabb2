// Generic small fused ReLU MLP on fp32 MFMA: forward (inference / SAVE), backward chain, weight and bias gradients (DESIGN.md section 2.13).
// Needs nerf_train_backward.hip.inc ahead of it (wgrad_impl); mfma32 comes from nerf_mlp_common.h.  The C surface is
// include/nerf_mi355x_nn.h.  fp32 throughout; the unit is compiled with -ffp-contract=off and every fused multiply-add here is an MFMA.
//
//     h_0 = relu(W_0 x + b_0),  h_i = relu(W_i h_{i-1} + b_i)  (i < n_hidden),  z = W_out h_last + b_out,  y = z or sigmoid(z)
//
// Layout.  A wave owns 32 points, the point on the lane index (lane l: point p = l & 31, half h = l >> 5), and a workgroup is four
// such waves.  v_mfma_f32_32x32x2_f32 computes D[32 out-features][32 points]: register r of out-tile t of lane (p, h) is feature
// act_feat(t, r, h) = 32 t + (r & 3) + 8 (r >> 2) + 4 h of point p -- and read as the B operand of the next layer that same register
// is the k-pair of k-step 16 t + r.  A layer's output is therefore the next layer's input as it stands (section 2.1); only the A
// operand (the weights) has to be read in that feature order.
//
// Weights.  The kernels read the nn.Linear tensors themselves (host arrays of device pointers travel in the kernel arguments): no
// packed copy exists.  A layer is staged through LDS in chunks of 64 reduction indices, once per workgroup, with coalesced loads
// (forward: 256 contiguous bytes of one weight row per wave-load; transposed product: two 128-byte row segments), and written to LDS
// in the order the MFMA consumes it: row m (the A operand's M index) holds, for lane-half h, the 32 k-steps of the chunk
// contiguously, so a lane fetches the A values of four k-steps with one 16-byte LDS read.  A row is 64 + 4 floats: the pad keeps the
// 16-byte reads of 16 neighbouring rows on distinct banks.  Everything that is not there (rows >= n_out, reduction indices >= n_in)
// is staged as 0.0f: padding happens in LDS and registers, no load reaches past a row or a tensor.
//
// The transposed product of the backward chain, dz_i = (W_{i+1}^T dz_{i+1}) * (h_i > 0), is the same GEMM with the other index of W on
// the rows: only the staging differs.  dz and grad_x are written, never accumulated, in a fixed order: bit-reproducible.

#include "../../include/nerf_mi355x_nn.h"
#include "nerf_host.h"
#include "nerf_mlp_common.h"

namespace {

constexpr int kFmBlock = 256;                  // 4 waves
constexpr int kFmWgPts = 128;                  // 32 points per wave
constexpr int kFmKC = 64;                      // reduction indices per staged chunk (32 k-steps)
constexpr int kFmRS = kFmKC + 4;               // floats per LDS row
constexpr int kFmMaxLayers = 9;                // n_hidden <= 8, plus the output layer

struct FmFwdArgs {
  const float* w[kFmMaxLayers];
  const float* b[kFmMaxLayers];
  const float* x;
  float* out;
  float* save;
  long long B;
  int in_dim, n_hidden, out_dim, activation;
  int x_vec4;                                  // x rows are whole, 16-byte aligned float4s
};

struct FmBwdArgs {
  const float* w[kFmMaxLayers];
  const float* out;
  const float* grad_out;
  const float* save;
  float* gsave;
  float* grad_x;
  long long B;
  int in_dim, n_hidden, out_dim, activation;
};

// where reduction index kk (0..63) of a chunk sits in an LDS row: [half h][k-step 16 t + r], kk = act_feat(t, r, h)
__device__ __forceinline__ int fm_slot(int kk) {
  const int m = kk & 31;
  return ((m >> 2) & 1) * 32 + (kk >> 5) * 16 + (m & 3) + 4 * (m >> 3);
}

// rows [0, rows) x reduction [kc, kc + 64) of W [n_out, n_in] -> LDS; row = output feature, reduction = input feature
__device__ __forceinline__ void fm_stage_fwd(float* __restrict__ lds, const float* __restrict__ W, int n_out, int n_in, int kc, int rows,
                                             int tid) {
  const int kk = tid & 63, k = kc + kk, slot = fm_slot(kk);
  const bool kok = k < n_in;
#pragma unroll 8
  for (int o = tid >> 6; o < rows; o += kFmBlock / 64)
    lds[o * kFmRS + slot] = (kok && o < n_out) ? W[(size_t)o * n_in + k] : 0.0f;
}

// the transposed operand: rows [m0, m0 + 32 mtiles) are INPUT features of W [n_out, n_in], the reduction [oc, oc + 64) its outputs
__device__ __forceinline__ void fm_stage_bwd(float* __restrict__ lds, const float* __restrict__ W, int n_out, int n_in, int m0, int oc,
                                             int mtiles, int tid) {
  const int mm = tid & 31;
  for (int jt = 0; jt < mtiles; ++jt) {
    const int m = m0 + 32 * jt + mm;
    const bool mok = m < n_in;
#pragma unroll 8
    for (int oo = tid >> 5; oo < kFmKC; oo += kFmBlock / 32)
      lds[(32 * jt + mm) * kFmRS + fm_slot(oo)] = (mok && oc + oo < n_out) ? W[(size_t)(oc + oo) * n_in + m] : 0.0f;
  }
}

// acc[j] += A(rows 32 j ..) * B for the staged chunk; b0 / b1 hold the chunk's two 32-wide reduction tiles in accumulator layout.
// ktiles (1 or 2, wave-uniform): how many of them hold anything
template <int MT, int NACC>
__device__ __forceinline__ void fm_gemm(const float* __restrict__ lds, int p, int h, int ktiles, const f32x16& b0, const f32x16& b1,
                                        f32x16 (&acc)[NACC]) {
  static_assert(MT <= NACC, "tiles");
  const float* __restrict__ base = lds + p * kFmRS + h * 32;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < ktiles) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          const float4 a = *reinterpret_cast<const float4*>(base + j * 32 * kFmRS + 16 * t + 4 * q);
          const f32x16& b = t ? b1 : b0;
          acc[j] = mfma32(a.x, b[4 * q + 0], acc[j]);
          acc[j] = mfma32(a.y, b[4 * q + 1], acc[j]);
          acc[j] = mfma32(a.z, b[4 * q + 2], acc[j]);
          acc[j] = mfma32(a.w, b[4 * q + 3], acc[j]);
        }
      }
    }
  }
}

// accumulator init = bias (features >= n_out: 0)
template <int NT>
__device__ __forceinline__ void fm_bias(const float* __restrict__ b, int n_out, int h, f32x16 (&acc)[NT]) {
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = nerf::act_feat(j, r, h);
      acc[j][r] = f < n_out ? b[f] : 0.0f;
    }
}

// one point's post-ReLU row -> block[row, :], four consecutive features per store (the block is 16-byte aligned, WIDTH % 32 == 0)
template <int NT>
__device__ __forceinline__ void fm_store_row(float* __restrict__ dst, int h, const f32x16 (&v)[NT]) {
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(dst + 32 * j + 8 * g + 4 * h) = make_float4(v[j][4 * g], v[j][4 * g + 1], v[j][4 * g + 2], v[j][4 * g + 3]);
}

template <int WIDTH, bool SAVE>
__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_fwd_kernel(FmFwdArgs a) {
  constexpr int NT = WIDTH / 32;
  __shared__ __attribute__((aligned(16))) float lds[WIDTH * kFmRS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
  const long long row = ((long long)blockIdx.x * (kFmBlock / 64) + wave) * 32 + p;
  const bool live = row < a.B;                 // dead rows compute on zeros and store nothing; every wave takes every barrier
  f32x16 acc[NT], act[NT];

  // layer 0: x is read from memory in accumulator order, 64 input features at a time
  fm_bias<NT>(a.b[0], WIDTH, h, acc);
  const float* __restrict__ xr = a.x + (size_t)(live ? row : 0) * a.in_dim;
  for (int kc = 0; kc < a.in_dim; kc += kFmKC) {
    f32x16 xb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = kc + 32 * t + 8 * g + 4 * h;           // features k0 .. k0 + 3 = act_feat(t, 4 g .. 4 g + 3, h)
        if (a.x_vec4) {
          const float4 v = (live && k0 < a.in_dim) ? *reinterpret_cast<const float4*>(xr + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
          xb[t][4 * g] = v.x; xb[t][4 * g + 1] = v.y; xb[t][4 * g + 2] = v.z; xb[t][4 * g + 3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) xb[t][4 * g + e] = (live && k0 + e < a.in_dim) ? xr[k0 + e] : 0.0f;
        }
      }
    __syncthreads();                            // the previous chunk has been consumed
    fm_stage_fwd(lds, a.w[0], WIDTH, a.in_dim, kc, WIDTH, tid);
    __syncthreads();
    fm_gemm<NT>(lds, p, h, a.in_dim - kc > 32 ? 2 : 1, xb[0], xb[1], acc);
  }

  for (int i = 0;; ++i) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) act[j][r] = fmaxf(acc[j][r], 0.0f);
    if (SAVE && live) fm_store_row<NT>(a.save + ((size_t)i * a.B + row) * WIDTH, h, act);
    if (i + 1 == a.n_hidden) break;
    fm_bias<NT>(a.b[i + 1], WIDTH, h, acc);
#pragma unroll
    for (int c = 0; c < WIDTH / kFmKC; ++c) {
      __syncthreads();
      fm_stage_fwd(lds, a.w[i + 1], WIDTH, WIDTH, c * kFmKC, WIDTH, tid);
      __syncthreads();
      fm_gemm<NT>(lds, p, h, 2, act[2 * c], act[2 * c + 1], acc);
    }
  }

  // output layer: one 32-row tile, rows >= out_dim are zeros in LDS
  f32x16 z[1];
  fm_bias<1>(a.b[a.n_hidden], a.out_dim, h, z);
#pragma unroll
  for (int c = 0; c < WIDTH / kFmKC; ++c) {
    __syncthreads();
    fm_stage_fwd(lds, a.w[a.n_hidden], a.out_dim, WIDTH, c * kFmKC, 32, tid);
    __syncthreads();
    fm_gemm<1>(lds, p, h, 2, act[2 * c], act[2 * c + 1], z);
  }
  if (live) {
    float* __restrict__ o = a.out + (size_t)row * a.out_dim;
#pragma unroll
    for (int r = 0; r < 8; ++r) {               // features 0..15 sit in registers 0..7
      const int f = nerf::act_feat(0, r, h);
      if (f < a.out_dim) o[f] = a.activation ? 1.0f / (1.0f + expf(-z[0][r])) : z[0][r];
    }
  }
}

template <int WIDTH>
__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_bwd_kernel(FmBwdArgs a) {
  constexpr int NT = WIDTH / 32;
  __shared__ __attribute__((aligned(16))) float lds[128 * kFmRS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
  const long long row = ((long long)blockIdx.x * (kFmBlock / 64) + wave) * 32 + p;
  const bool live = row < a.B;
  const size_t plane = (size_t)a.B * WIDTH;    // one [B, WIDTH] block of save / gsave

  // dz_out in accumulator layout (tile 0, features 0..15 in registers 0..7), and into the last block of gsave
  f32x16 dzo;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int f = nerf::act_feat(0, r, h);
    float g = 0.0f;
    if (r < 8 && live && f < a.out_dim) {
      const size_t at = (size_t)row * a.out_dim + f;
      g = a.grad_out[at];
      if (a.activation) { const float y = a.out[at]; g = (g * y) * (1.0f - y); }
      a.gsave[(size_t)a.n_hidden * plane + at] = g;
    }
    dzo[r] = g;
  }

  f32x16 acc[NT], dz[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) dz[j][r] = 0.0f;
  for (int i = a.n_hidden - 1; i >= 0; --i) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    if (i == a.n_hidden - 1) {                  // from the output layer: out_dim <= 16 outputs, one half-filled chunk
      __syncthreads();
      fm_stage_bwd(lds, a.w[i + 1], a.out_dim, WIDTH, 0, 0, NT, tid);
      __syncthreads();
      fm_gemm<NT>(lds, p, h, 1, dzo, dzo, acc);
    } else {
#pragma unroll
      for (int c = 0; c < WIDTH / kFmKC; ++c) {
        __syncthreads();
        fm_stage_bwd(lds, a.w[i + 1], WIDTH, WIDTH, 0, c * kFmKC, NT, tid);
        __syncthreads();
        fm_gemm<NT>(lds, p, h, 2, dz[2 * c], dz[2 * c + 1], acc);
      }
    }
    // the ReLU mask from the saved row: exactly 0 where h_i is 0
    const float* __restrict__ hrow = a.save + (size_t)i * plane + (size_t)(live ? row : 0) * WIDTH;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 hv = live ? *reinterpret_cast<const float4*>(hrow + 32 * j + 8 * g + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
        dz[j][4 * g + 0] = hv.x > 0.0f ? acc[j][4 * g + 0] : 0.0f;
        dz[j][4 * g + 1] = hv.y > 0.0f ? acc[j][4 * g + 1] : 0.0f;
        dz[j][4 * g + 2] = hv.z > 0.0f ? acc[j][4 * g + 2] : 0.0f;
        dz[j][4 * g + 3] = hv.w > 0.0f ? acc[j][4 * g + 3] : 0.0f;
      }
    if (live) fm_store_row<NT>(a.gsave + (size_t)i * plane + (size_t)row * WIDTH, h, dz);
  }

  if (a.grad_x == nullptr) return;              // (kernel argument: the whole grid leaves together)
  // grad_x = W_0^T dz_0, 64 input features at a time
  for (int m0 = 0; m0 < a.in_dim; m0 += 64) {
    const int mtiles = a.in_dim - m0 > 32 ? 2 : 1;
    f32x16 gx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gx[j][r] = 0.0f;
#pragma unroll
    for (int c = 0; c < WIDTH / kFmKC; ++c) {
      __syncthreads();
      fm_stage_bwd(lds, a.w[0], WIDTH, a.in_dim, m0, c * kFmKC, mtiles, tid);
      __syncthreads();
      if (mtiles == 2) fm_gemm<2>(lds, p, h, 2, dz[2 * c], dz[2 * c + 1], gx);
      else fm_gemm<1>(lds, p, h, 2, dz[2 * c], dz[2 * c + 1], gx);
    }
    if (live) {
      float* __restrict__ gr = a.grad_x + (size_t)row * a.in_dim + m0;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f = nerf::act_feat(j, r, h);
          if (j < mtiles && m0 + f < a.in_dim) gr[f] = gx[j][r];
        }
    }
  }
}

// Bias gradients of all layers in one launch: db_i[o] += sum_p dz_i[p, o].  blockIdx.y is the layer, blockIdx.x a range of
// kFmBiasRows rows.  A block walks its rows as one flat array with a stride of the largest multiple of n_out within 256, so a thread
// stays on column t % n_out and consecutive threads read consecutive floats; it sums in float64, the threads of a column are added up in float64
// through LDS, and the block's sum is rounded ONCE and added to db with one atomic per column.  (The weight-gradient kernels can sum
// a bias as well, but in fp32 and row after row: the float64 partial sums here keep a bias gradient of any batch within a few ulps of
// the exact sum -- what remains is the rounding of one fp32 atomic add per 1024 rows.)
constexpr int kFmBiasRows = 1024;

struct FmBiasArgs {
  const float* dz[kFmMaxLayers];
  float* db[kFmMaxLayers];
  int n_out[kFmMaxLayers];
  long long B;
};

__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_bias_grad_kernel(FmBiasArgs a) {
  __shared__ double part[kFmBlock];
  const int layer = blockIdx.y, n_out = a.n_out[layer], tid = threadIdx.x;
  float* __restrict__ db = a.db[layer];
  if (db == nullptr) return;                   // (block-uniform)
  const long long r0 = (long long)blockIdx.x * kFmBiasRows;
  const long long r1 = r0 + kFmBiasRows < a.B ? r0 + kFmBiasRows : a.B;
  const float* __restrict__ dz = a.dz[layer] + r0 * n_out;
  const long long n = (r1 - r0) * n_out;       // <= 1024 * 128 elements
  const int stride = kFmBlock / n_out * n_out;  // the threads below it walk the block's elements; a multiple of n_out (<= 128)
  double sum = 0.0;
  if (tid < stride)
    for (long long e = tid; e < n; e += stride) sum += (double)dz[e];
  part[tid] = sum;
  __syncthreads();
  if (tid < n_out) {
    double total = 0.0;
    for (int t = tid; t < stride; t += n_out) total += part[t];
    atomicAdd(db + tid, (float)total);
  }
}

// ---- host side

constexpr long long kFmMaxIndex = 0x7fffffffLL;               // B * max(in_dim, width) stays below 2^31: one launch, chunk above it

bool fm_domain(int64_t B, int32_t width, int32_t n_hidden, int32_t out_dim) {
  return B >= 1 && (width == 64 || width == 128) && n_hidden >= 1 && n_hidden <= 8 && out_dim >= 1 && out_dim <= 16 &&
         B <= kFmMaxIndex / 256;
}

// everything both entries check before a launch
int fm_check(const char* entry, int64_t B, int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim, int32_t activation) {
  if (width != 64 && width != 128) return fail(NERF_ERR_UNSUPPORTED, "%s: width must be 64 or 128", entry);
  if (n_hidden < 1 || n_hidden > 8) return fail(NERF_ERR_UNSUPPORTED, "%s: n_hidden must be 1..8", entry);
  if (out_dim < 1 || out_dim > 16) return fail(NERF_ERR_UNSUPPORTED, "%s: out_dim must be 1..16", entry);
  if (in_dim < 1 || in_dim > 256) return fail(NERF_ERR_UNSUPPORTED, "%s: in_dim must be 1..256", entry);
  if (activation != NERF_NN_ACT_NONE && activation != NERF_NN_ACT_SIGMOID)
    return fail(NERF_ERR_UNSUPPORTED, "%s: activation must be 0 (none) or 1 (sigmoid)", entry);
  if (B <= 0) return fail(NERF_ERR_INVALID_ARG, "%s: the batch must be positive", entry);
  if (B > kFmMaxIndex / 256) return fail(NERF_ERR_INVALID_ARG, "%s: more than 8 388 607 rows: run the batch in chunks", entry);
  return NERF_OK;
}

bool fm_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// everything nerf_fused_mlp_backward checks before a launch (nerf_fused_mlp_backward_exact checks the same); fills the chain
// kernel's arguments
int fm_bwd_check(const char* entry, const float* x, const float* out, const float* grad_out, int64_t B, int32_t in_dim, int32_t width,
                 int32_t n_hidden, int32_t out_dim, int32_t activation, const float* const weights[], const float* save, float* gsave,
                 float* const grad_weights[], float* const grad_biases[], float* grad_x, FmBwdArgs& a) {
  int rc = fm_check(entry, B, in_dim, width, n_hidden, out_dim, activation);
  if (rc) return rc;
  if (!x || !grad_out || !weights || !save || !gsave || !grad_weights || !grad_biases || (activation && !out))
    return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!fm_aligned(x, 4) || !fm_aligned(out, 4) || !fm_aligned(grad_out, 4) || !fm_aligned(grad_x, 4) || !fm_aligned(save, 16) ||
      !fm_aligned(gsave, 16))
    return fail(NERF_ERR_INVALID_ARG, "%s: x, out, grad_out and grad_x must be aligned to 4 bytes, save and gsave to 16", entry);
  a = {};
  for (int i = 0; i <= n_hidden; ++i) {
    if (!weights[i]) return fail(NERF_ERR_INVALID_ARG, "%s: null parameter pointer", entry);
    if (!fm_aligned(weights[i], 4) || !fm_aligned(grad_weights[i], 4) || !fm_aligned(grad_biases[i], 4))
      return fail(NERF_ERR_INVALID_ARG, "%s: misaligned parameter or gradient pointer", entry);
    a.w[i] = weights[i];
  }
  a.out = out; a.grad_out = grad_out; a.save = save; a.gsave = gsave; a.grad_x = grad_x; a.B = B;
  a.in_dim = in_dim; a.n_hidden = n_hidden; a.out_dim = out_dim; a.activation = activation;
  return NERF_OK;
}

// the gradient chain: gsave and grad_x
int fm_bwd_chain(const FmBwdArgs& a, int32_t width, void* stream) {
  const dim3 grid((unsigned)((a.B + kFmWgPts - 1) / kFmWgPts)), blk(kFmBlock);
  hipStream_t st = (hipStream_t)stream;
  return width == 64 ? NERF_LAUNCH(nerf_fused_mlp_bwd_kernel<64>, grid, blk, st, a) : NERF_LAUNCH(nerf_fused_mlp_bwd_kernel<128>, grid, blk, st, a);
}

}  // namespace

extern "C" {

int32_t nerf_nn_abi_version(void) { return NERF_NN_ABI_VERSION; }

int64_t nerf_fused_mlp_save_floats(int64_t B, int32_t width, int32_t n_hidden) {
  if (!fm_domain(B, width, n_hidden, 1)) return -1;
  return (int64_t)n_hidden * B * width;
}

int64_t nerf_fused_mlp_grad_floats(int64_t B, int32_t width, int32_t n_hidden, int32_t out_dim) {
  if (!fm_domain(B, width, n_hidden, out_dim)) return -1;
  return (int64_t)n_hidden * B * width + B * out_dim;
}

int32_t nerf_fused_mlp_forward(const float* x, int64_t B, int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim,
                               int32_t activation, const float* const weights[], const float* const biases[], float* out, float* save,
                               void* stream) {
  const char* entry = "nerf_fused_mlp_forward";
  int rc = fm_check(entry, B, in_dim, width, n_hidden, out_dim, activation);
  if (rc) return rc;
  if (!x || !weights || !biases || !out) return fail(NERF_ERR_INVALID_ARG, "%s: null argument", entry);
  if (!fm_aligned(x, 4) || !fm_aligned(out, 4) || !fm_aligned(save, 16))
    return fail(NERF_ERR_INVALID_ARG, "%s: x and out must be aligned to 4 bytes, save to 16", entry);
  FmFwdArgs a = {};
  for (int i = 0; i <= n_hidden; ++i) {
    if (!weights[i] || !biases[i]) return fail(NERF_ERR_INVALID_ARG, "%s: null parameter pointer", entry);
    if (!fm_aligned(weights[i], 4) || !fm_aligned(biases[i], 4)) return fail(NERF_ERR_INVALID_ARG, "%s: misaligned parameter pointer", entry);
    a.w[i] = weights[i]; a.b[i] = biases[i];
  }
  a.x = x; a.out = out; a.save = save; a.B = B;
  a.in_dim = in_dim; a.n_hidden = n_hidden; a.out_dim = out_dim; a.activation = activation;
  a.x_vec4 = in_dim % 4 == 0 && fm_aligned(x, 16);
  const dim3 grid((unsigned)((B + kFmWgPts - 1) / kFmWgPts)), blk(kFmBlock);
  hipStream_t st = (hipStream_t)stream;
  if (width == 64)
    return save ? NERF_LAUNCH((nerf_fused_mlp_fwd_kernel<64, true>), grid, blk, st, a)
                : NERF_LAUNCH((nerf_fused_mlp_fwd_kernel<64, false>), grid, blk, st, a);
  return save ? NERF_LAUNCH((nerf_fused_mlp_fwd_kernel<128, true>), grid, blk, st, a)
              : NERF_LAUNCH((nerf_fused_mlp_fwd_kernel<128, false>), grid, blk, st, a);
}

int32_t nerf_fused_mlp_backward(const float* x, const float* out, const float* grad_out, int64_t B, int32_t in_dim, int32_t width,
                                int32_t n_hidden, int32_t out_dim, int32_t activation, const float* const weights[], const float* save,
                                float* gsave, float* const grad_weights[], float* const grad_biases[], float* grad_x, void* stream) {
  FmBwdArgs a;
  int rc = fm_bwd_check("nerf_fused_mlp_backward", x, out, grad_out, B, in_dim, width, n_hidden, out_dim, activation, weights, save, gsave,
                        grad_weights, grad_biases, grad_x, a);
  if (rc) return rc;
  rc = fm_bwd_chain(a, width, stream);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kFmBlock);
  // weight gradients: dW_i += dz_i^T in_i, one nerf_wgrad launch per layer that wants them; bias gradients: db_i += sum_p dz_i, one
  // launch for all layers
  const int64_t plane = B * width;
  FmBiasArgs ba = {};
  bool any_bias = false;
  for (int i = 0; i <= n_hidden; ++i) {
    const int n_out = i < n_hidden ? width : out_dim, n_in = i ? width : in_dim;
    ba.dz[i] = gsave + i * plane; ba.db[i] = grad_biases[i]; ba.n_out[i] = n_out;
    any_bias = any_bias || grad_biases[i];
    if (!grad_weights[i]) continue;
    rc = wgrad_impl(gsave + i * plane, n_out, 0, n_out, i ? save + (i - 1) * plane : x, n_in, 0, n_in, grad_weights[i], n_in, 0,
                    nullptr, B, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  if (!any_bias) return NERF_OK;
  ba.B = B;
  return NERF_LAUNCH(nerf_fused_mlp_bias_grad_kernel, dim3((unsigned)((B + kFmBiasRows - 1) / kFmBiasRows), (unsigned)(n_hidden + 1)),
                     blk, st, ba);
}

}  // extern "C"
