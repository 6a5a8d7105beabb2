// Fused MLP: exact, order-independent weight and bias gradients (DESIGN.md section 2.13.1; include/nerf_mi355x_nn_exact.h has the
// contract).  Needs nerf_fused_mlp.hip.inc ahead of it: the gradient chain (gsave, grad_x) is that file's kernel, unchanged.  The sums
//     dW_i[o,k] += sum_p fmul(dz_i[p,o], in_i[p,k])        db_i[o] += sum_p dz_i[p,o]
// are taken in 64-bit fixed point (nerf_fixed_sum.h) instead of with fp32 atomics, in four passes over a zero-filled workspace:
//   column maxima   A[o] = max_p |dz_i[p,o]|, H[k] = max_p |in_i[p,k]| as bit patterns      one no-return uint32 atomic max per column
//                                                                                            and workgroup, every operand block in ONE launch
//   bias add        accb[o]   += q(dz_i[p,o], e(A[o]))                                       one no-return int64 atomic add per column
//   weight add      acc[o,k]  += q(fmul(dz_i[p,o], in_i[p,k]), e(fmul(A[o], H[k])))          ... per element and workgroup, one launch per layer
//   finish          grad += value(acc, emax), every wanted element of every layer           flat, plain loads and stores
// The scale of an element comes from the column maxima (fx_product_exponent), not from its largest term: no pass over the B * n_out *
// n_in products is needed to find it, and the add and the finish pass recompute it from the same two words.  Integer max and add do
// not depend on the arrival order: the bytes are the same from run to run and under any permutation of the rows.  No inline asm, no
// MFMA (an fp32 MFMA rounds inside its accumulator).
#include "../../include/nerf_mi355x_nn_exact.h"
#include "nerf_host.h"
#include "nerf_fixed_sum.h"

namespace {

constexpr int kFxColRows = 1024;               // rows per workgroup of the column passes (maxima, bias add)
constexpr int kFxRows = 1024;                  // rows per workgroup of the weight add: 8 bytes of atomics per element per 1024 rows
constexpr int kFxTile = 64;                    // a workgroup's tile: 64 outputs x 64 inputs, 4 x 4 elements per thread
constexpr int kFxChunk = 32;                   // rows staged in LDS at a time
constexpr int kFxMaxBlocks = 2 * kFmMaxLayers; // operand blocks: x, n_hidden x save, (n_hidden + 1) x gsave

// where everything sits in the workspace, in elements: int64 acc = per layer its weights [n_out * n_in] then its bias [n_out];
// behind all of them uint32 colmax = x [in_dim], save [n_hidden * width], gsave [n_hidden * width + out_dim]
struct FxLayout {
  int64_t acc_w[kFmMaxLayers], acc_b[kFmMaxLayers], acc_total;
  int64_t max_in[kFmMaxLayers], max_dz[kFmMaxLayers], max_total;
  int n_out[kFmMaxLayers], n_in[kFmMaxLayers];
  int64_t bytes() const { return align256(8 * acc_total + 4 * max_total); }
};

FxLayout fx_layout(int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim) {
  FxLayout l = {};
  for (int i = 0; i <= n_hidden; ++i) {
    l.n_out[i] = i < n_hidden ? width : out_dim;
    l.n_in[i] = i ? width : in_dim;
    l.acc_w[i] = l.acc_total; l.acc_total += (int64_t)l.n_out[i] * l.n_in[i];
    l.acc_b[i] = l.acc_total; l.acc_total += l.n_out[i];
  }
  for (int i = 0; i <= n_hidden; ++i) { l.max_in[i] = l.max_total; l.max_total += l.n_in[i]; }
  for (int i = 0; i <= n_hidden; ++i) { l.max_dz[i] = l.max_total; l.max_total += l.n_out[i]; }
  return l;
}

bool fx_domain(int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim) {
  return fm_domain(1, width, n_hidden, out_dim) && in_dim >= 1 && in_dim <= 256;
}

// ---- column passes.  blockIdx.y is the operand block (or the layer), blockIdx.x a range of kFxColRows rows.  A workgroup walks its
// rows as one flat array with a stride of the largest multiple of the column count within 256 (nerf_fused_mlp_bias_grad_kernel's
// walk): a thread stays on one column, consecutive threads read consecutive floats; the threads of a column meet in LDS.
struct FxColArgs {
  const float* src[kFxMaxBlocks];              // [B, cols] row-major; NULL: no wanted gradient reads the block (maxima) / bias not wanted
  uint32_t* colmax[kFxMaxBlocks];              // [cols]
  unsigned long long* acc[kFmMaxLayers];       // bias add only: [cols]
  int cols[kFxMaxBlocks];
  long long B;
  int K;
};

__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_exact_colmax_kernel(FxColArgs a) {
  __shared__ uint32_t part[kFmBlock];
  const int blk = blockIdx.y, tid = threadIdx.x, n = a.cols[blk];
  if (a.src[blk] == nullptr) return;           // (block-uniform)
  const long long r0 = (long long)blockIdx.x * kFxColRows;
  const long long r1 = r0 + kFxColRows < a.B ? r0 + kFxColRows : a.B;
  const float* __restrict__ src = a.src[blk] + r0 * n;
  const int count = (int)(r1 - r0) * n;        // <= 1024 * 256
  const int stride = kFmBlock / n * n;
  uint32_t m = 0u;
  if (tid < stride)
#pragma unroll 4
    for (int e = tid; e < count; e += stride) {
      const uint32_t v = __float_as_uint(src[e]) & 0x7fffffffu;
      m = v > m ? v : m;
    }
  part[tid] = m;
  __syncthreads();
  if (tid < n) {
    uint32_t top = 0u;
    for (int t = tid; t < stride; t += n) top = part[t] > top ? part[t] : top;
    if (top != 0u) atomicMax(a.colmax[blk] + tid, top);       // result unused: the no-return form; a column of zeros asks for nothing
  }
}

__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_exact_bias_kernel(FxColArgs a) {
  __shared__ long long part[kFmBlock];
  const int layer = blockIdx.y, tid = threadIdx.x, n = a.cols[layer];
  if (a.src[layer] == nullptr) return;         // (block-uniform)
  const long long r0 = (long long)blockIdx.x * kFxColRows;
  const long long r1 = r0 + kFxColRows < a.B ? r0 + kFxColRows : a.B;
  const float* __restrict__ src = a.src[layer] + r0 * n;
  const int count = (int)(r1 - r0) * n;
  const int stride = kFmBlock / n * n;
  long long sum = 0;
  if (tid < stride) {
    const uint32_t top = fx_exponent(a.colmax[layer][tid % n]);            // complete: the maxima pass ended before this kernel began
#pragma unroll 4
    for (int e = tid; e < count; e += stride) {
      const uint32_t bits = __float_as_uint(src[e]);
      if (fx_exponent(bits) != 0u) sum += fx_quantize(bits, top, a.K);      // (top == 255: the finish pass ignores the sum)
    }
  }
  part[tid] = sum;
  __syncthreads();
  if (tid < n) {
    long long total = 0;
    for (int t = tid; t < stride; t += n) total += part[t];
    if (total != 0) atomicAdd(a.acc[layer] + tid, (unsigned long long)total);   // two's complement; result unused
  }
}

// Liveness in the two add kernels.  The contract's live terms have 1 <= e <= 254; the kernels test e != 0 only.  A poison term
// (e == 255: Inf or NaN) can only occur where the element's top is 255 as well: a NaN or Inf operand is its column's maximum (a NaN
// outranks everything), and its product with the other column's maximum -- even with 0 -- has the exponent 255; an overflowing
// product of finite operands is at most fmul(A, H), which then overflows too.  For such an element the finish pass writes the NaN
// and never reads the accumulator, so what a poison term adds to it (fx_quantize with s = 0) is never seen, and the test for 255
// is left out of the inner loops.  Padding elements get top = 255 for the same reason, and are never stored.

// ---- weight add.  grid = (row ranges, input tiles, output tiles) of ONE layer.  Thread (to, tk) = (tid / 16, tid % 16) owns outputs
// o0 + 4 to + i and inputs k0 + tk + 16 j (i, j = 0..3): for fixed (i, j) the 16 lanes of a `to` land on 16 consecutive elements, a
// wave's atomic instruction on four 128-byte segments.  Rows pass through LDS 32 at a time, each read from memory once per workgroup;
// the input columns are stored permuted (column c at slot 4 (c % 16) + c / 16) so that a thread's four are one 16-byte read.
// Everything outside the layer or the row range is staged as 0.0f: a null term.
struct FxAddArgs {
  const float* dz;                             // [B, n_out]
  const float* in;                             // [B, n_in]
  const uint32_t* amax;                        // [n_out]
  const uint32_t* hmax;                        // [n_in]
  unsigned long long* acc;                     // [n_out, n_in]
  long long B;
  int n_out, n_in, K;
};

__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_exact_add_kernel(FxAddArgs a) {
  __shared__ __attribute__((aligned(16))) float dzs[kFxChunk][kFxTile];
  __shared__ __attribute__((aligned(16))) float ins[kFxChunk][kFxTile];
  const int tid = threadIdx.x, to = tid >> 4, tk = tid & 15;
  const int k0 = blockIdx.y * kFxTile, o0 = blockIdx.z * kFxTile;
  const long long r0 = (long long)blockIdx.x * kFxRows;
  const long long r1 = r0 + kFxRows < a.B ? r0 + kFxRows : a.B;

  // emax of the thread's elements.  Outside the layer: 255, so that a NaN or Inf dz meeting a padding zero (its product has the
  // exponent 255) still shifts by a defined amount; nothing of such an element is ever stored
  uint32_t top[4][4];
  {
    uint32_t am[4], hm[4];                     // complete: the maxima pass ended before this kernel began
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = o0 + 4 * to + i;
      am[i] = o < a.n_out ? a.amax[o] : 0x7fc00000u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + tk + 16 * j;
      hm[j] = k < a.n_in ? a.hmax[k] : 0x7fc00000u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) top[i][j] = fx_product_exponent(am[i], hm[j]);
  }
  long long acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;

  // staging: thread tid moves column tid % 64 of rows tid / 64 + 4 n.  Every load is issued, from an address clamped into the
  // thread's last live row and the layer's last column, and what lies outside is replaced by 0.0f afterwards: the 16 loads of a
  // chunk are in flight together and none reaches past a row or the batch
  const int c = tid & 63;
  const bool o_ok = o0 + c < a.n_out, k_ok = k0 + c < a.n_in;
  const int oc = o_ok ? o0 + c : a.n_out - 1, kc = k_ok ? k0 + c : a.n_in - 1;
  for (long long rc = r0; rc < r1; rc += kFxChunk) {
    const int rows = r1 - rc < kFxChunk ? (int)(r1 - rc) : kFxChunk;
    float dv[kFxChunk / 4], hv[kFxChunk / 4];
#pragma unroll
    for (int n = 0; n < kFxChunk / 4; ++n) {
      const int r = (tid >> 6) + 4 * n;
      const size_t row = (size_t)(rc + (r < rows ? r : rows - 1));
      dv[n] = a.dz[row * a.n_out + oc];
      hv[n] = a.in[row * a.n_in + kc];
    }
    __syncthreads();                            // the previous chunk has been consumed
#pragma unroll
    for (int n = 0; n < kFxChunk / 4; ++n) {
      const int r = (tid >> 6) + 4 * n;
      dzs[r][c] = (r < rows && o_ok) ? dv[n] : 0.0f;
      ins[r][4 * (c & 15) + (c >> 4)] = (r < rows && k_ok) ? hv[n] : 0.0f;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const float4 d4 = *reinterpret_cast<const float4*>(&dzs[r][4 * to]);
      const float4 h4 = *reinterpret_cast<const float4*>(&ins[r][4 * tk]);
      const float d[4] = {d4.x, d4.y, d4.z, d4.w}, h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((__float_as_uint(d[i]) << 1) == 0u) continue;      // a ReLU zero (or padding): four null terms at once
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t bits = __float_as_uint(d[i] * h[j]);   // the term: one fp32 multiplication (the unit is built with -ffp-contract=off)
          if (fx_exponent(bits) != 0u) acc[i][j] += fx_quantize(bits, top[i][j], a.K);   // (top == 255: the finish pass ignores the sum)
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = o0 + 4 * to + i, k = k0 + tk + 16 * j;
      if (o < a.n_out && k < a.n_in && acc[i][j] != 0)
        atomicAdd(a.acc + (size_t)o * a.n_in + k, (unsigned long long)acc[i][j]);    // two's complement; result unused
    }
}

// ---- finish: one thread per accumulator of the workspace, weights and bias of every layer in the workspace's order
struct FxFinishArgs {
  float* grad[2 * kFmMaxLayers];               // segment 2 i: the weights of layer i, 2 i + 1: its bias; NULL: not wanted, not touched
  const uint32_t* amax[2 * kFmMaxLayers];
  const uint32_t* hmax[2 * kFmMaxLayers];      // NULL: a bias segment
  int end[2 * kFmMaxLayers];                   // one past the segment's last accumulator
  int n_in[2 * kFmMaxLayers];                  // (1 for a bias segment)
  const unsigned long long* acc;
  int segments, K;
};

__global__ __launch_bounds__(kFmBlock)
void nerf_fused_mlp_exact_finish_kernel(FxFinishArgs a) {
  const int e = blockIdx.x * kFmBlock + threadIdx.x;
  int s = 0, first = 0;
  while (s < a.segments && e >= a.end[s]) first = a.end[s++];
  if (s == a.segments || a.grad[s] == nullptr) return;
  const int local = e - first, o = local / a.n_in[s], k = local % a.n_in[s];
  const uint32_t top = a.hmax[s] ? fx_product_exponent(a.amax[s][o], a.hmax[s][k]) : fx_exponent(a.amax[s][o]);
  if (top == 0u) return;                        // no live term: the element is neither read nor written
  float* __restrict__ g = a.grad[s] + local;
  *g = top == kFxPoison ? __uint_as_float(0x7fc00000u) : *g + fx_finish((long long)a.acc[e], top, a.K);
}

}  // namespace

extern "C" {

int64_t nerf_fused_mlp_exact_workspace_bytes(int32_t in_dim, int32_t width, int32_t n_hidden, int32_t out_dim) {
  if (!fx_domain(in_dim, width, n_hidden, out_dim)) return -1;
  return fx_layout(in_dim, width, n_hidden, out_dim).bytes();
}

int32_t nerf_fused_mlp_exact_guard_bits(int64_t B) {
  if (B < 1 || B > kFmMaxIndex / 256) return -1;
  return fx_guard_bits(B);
}

int32_t nerf_fused_mlp_backward_exact(const float* x, const float* out, const float* grad_out, int64_t B, int32_t in_dim, int32_t width,
                                      int32_t n_hidden, int32_t out_dim, int32_t activation, const float* const weights[],
                                      const float* save, float* gsave, float* const grad_weights[], float* const grad_biases[],
                                      float* grad_x, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* entry = "nerf_fused_mlp_backward_exact";
  FmBwdArgs chain;
  int rc = fm_bwd_check(entry, x, out, grad_out, B, in_dim, width, n_hidden, out_dim, activation, weights, save, gsave, grad_weights,
                        grad_biases, grad_x, chain);
  if (rc) return rc;
  if (!workspace || !fm_aligned(workspace, 16)) return fail(NERF_ERR_INVALID_ARG, "%s: the workspace must be given and aligned to 16 bytes", entry);
  const FxLayout l = fx_layout(in_dim, width, n_hidden, out_dim);
  if (workspace_bytes < l.bytes())
    return fail(NERF_ERR_WORKSPACE, "%s: the workspace is smaller than nerf_fused_mlp_exact_workspace_bytes(in_dim, width, n_hidden, out_dim)",
                entry);
  hipStream_t st = (hipStream_t)stream;
  rc = fm_bwd_chain(chain, width, stream);
  if (rc) return rc;

  unsigned long long* acc = (unsigned long long*)workspace;
  uint32_t* colmax = (uint32_t*)(acc + l.acc_total);
  const int64_t plane = B * width;
  const int K = fx_guard_bits(B);
  FxColArgs maxima = {}, bias = {};
  FxFinishArgs fin = {};
  bool any = false, any_bias = false;
  maxima.B = bias.B = B; maxima.K = bias.K = fin.K = K;
  fin.acc = acc; fin.segments = 2 * (n_hidden + 1);
  for (int i = 0; i <= n_hidden; ++i) {
    const float* in = i ? save + (i - 1) * plane : x;
    const float* dz = gsave + i * plane;
    const bool want_w = grad_weights[i], want_b = grad_biases[i];
    any = any || want_w || want_b; any_bias = any_bias || want_b;
    // operand block i: the layer's input rows, block n_hidden + 1 + i: its dz
    maxima.src[i] = want_w ? in : nullptr; maxima.colmax[i] = colmax + l.max_in[i]; maxima.cols[i] = l.n_in[i];
    const int d = n_hidden + 1 + i;
    maxima.src[d] = want_w || want_b ? dz : nullptr; maxima.colmax[d] = colmax + l.max_dz[i]; maxima.cols[d] = l.n_out[i];
    bias.src[i] = want_b ? dz : nullptr; bias.colmax[i] = colmax + l.max_dz[i]; bias.cols[i] = l.n_out[i]; bias.acc[i] = acc + l.acc_b[i];
    fin.grad[2 * i] = grad_weights[i]; fin.amax[2 * i] = colmax + l.max_dz[i]; fin.hmax[2 * i] = colmax + l.max_in[i];
    fin.end[2 * i] = (int)l.acc_b[i]; fin.n_in[2 * i] = l.n_in[i];
    fin.grad[2 * i + 1] = grad_biases[i]; fin.amax[2 * i + 1] = colmax + l.max_dz[i]; fin.hmax[2 * i + 1] = nullptr;
    fin.end[2 * i + 1] = (int)(l.acc_b[i] + l.n_out[i]); fin.n_in[2 * i + 1] = 1;
  }
  if (!any) return NERF_OK;
  if (hipMemsetAsync(workspace, 0, (size_t)(8 * l.acc_total + 4 * l.max_total), st) != hipSuccess)
    return fail(NERF_ERR_HIP, "%s: memset failed", entry);
  const dim3 blk(kFmBlock);
  const unsigned col_ranges = (unsigned)((B + kFxColRows - 1) / kFxColRows), ranges = (unsigned)((B + kFxRows - 1) / kFxRows);
  rc = NERF_LAUNCH(nerf_fused_mlp_exact_colmax_kernel, dim3(col_ranges, (unsigned)(2 * (n_hidden + 1))), blk, st, maxima);
  if (rc) return rc;
  if (any_bias) {
    rc = NERF_LAUNCH(nerf_fused_mlp_exact_bias_kernel, dim3(col_ranges, (unsigned)(n_hidden + 1)), blk, st, bias);
    if (rc) return rc;
  }
  for (int i = 0; i <= n_hidden; ++i) {
    if (!grad_weights[i]) continue;
    FxAddArgs add = {gsave + i * plane, i ? save + (i - 1) * plane : x, colmax + l.max_dz[i], colmax + l.max_in[i], acc + l.acc_w[i], B,
                     l.n_out[i], l.n_in[i], K};
    rc = NERF_LAUNCH(nerf_fused_mlp_exact_add_kernel,
                     dim3(ranges, (unsigned)((l.n_in[i] + kFxTile - 1) / kFxTile), (unsigned)((l.n_out[i] + kFxTile - 1) / kFxTile)), blk, st, add);
    if (rc) return rc;
  }
  return NERF_LAUNCH(nerf_fused_mlp_exact_finish_kernel, dim3((unsigned)((l.acc_total + kFmBlock - 1) / kFmBlock)), blk, st, fin);
}

}  // extern "C"
