#ifndef NERF_WG_HACK_NOATOMIC         // timing-only: the weight-gradient kernels drop their final atomic adds (wrong results)
#define NERF_WG_HACK_NOATOMIC 0
#endif
// Weight-gradient GEMM for the training path (fp32 MFMA): dW[o][i] += sum_p dZ[p][o] * Hin[p][i].
// (included by nerf_kernels.hip)
//
// This is what autograd computes for every nn.Linear of network.py:22-47 (grad_weight = grad_out^T @
// input, grad_bias = grad_out.sum(0)).  The reduction index is the POINT, so both MFMA operands want
// "feature on the lane, point on k": exactly what row-major [P, C] activations give (lanes 0-31 read
// 128 contiguous bytes of row 2s, lanes 32-63 of row 2s+1).  Workgroups are persistent over
// contiguous point ranges, each wave keeps OT x IT 32x32 output tiles in registers (4x4 = 256
// accumulators for a 256x256 layer split over the 4 waves) and adds them to dW with float atomics
// at the end (256-B row segments per wave-instruction, the full-rate shape).
struct WgradArgs {
  const float* dz; long long ldz; int zc0; int n_out;
  const float* hin; long long ldh; int hc0; int n_in;
  float* dw; long long ldw; int wc0;
  float* db;
  long long n_points;
  int osplit, isplit;      // how the 4 waves split the out / in tiles (osplit * isplit == 4)
  // LIST instances of the asm-ring kernels: the point range is the list of live 32-point tiles of the backward pass
  // (nerf_tile_flags_kernel / nerf_tile_scan_kernel); dead tiles hold no valid rows and are never read
  const int* live_tiles;
  const int* n_live;
};

template <int OT, int IT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad_f32_kernel(WgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wo = wave / a.isplit, wi = wave % a.isplit;
  const long long n_pairs = (a.n_points + 1) / 2;
  const long long per = (n_pairs + gridDim.x - 1) / gridDim.x;
  const long long s0 = (long long)blockIdx.x * per;
  long long s1 = s0 + per;
  if (s1 > n_pairs) s1 = n_pairs;

  int ocol[OT], icol[IT];
  bool ook[OT], iok[IT];
#pragma unroll
  for (int j = 0; j < OT; ++j) { ocol[j] = 32 * (wo * OT + j) + i; ook[j] = ocol[j] < a.n_out; }
#pragma unroll
  for (int j = 0; j < IT; ++j) { icol[j] = 32 * (wi * IT + j) + i; iok[j] = icol[j] < a.n_in; }

  f32x16 acc[OT][IT];
#pragma unroll
  for (int jo = 0; jo < OT; ++jo)
#pragma unroll
    for (int ji = 0; ji < IT; ++ji)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[jo][ji][r] = 0.0f;
  float bsum[OT];
#pragma unroll
  for (int j = 0; j < OT; ++j) bsum[j] = 0.0f;

  constexpr int PF = 4;                            // k-steps in flight
  float A[PF][OT], B[PF][IT];
  auto load = [&](long long s, float (&Av)[OT], float (&Bv)[IT]) {
    const long long row = 2 * s + h;
    const bool rok = s < s1 && row < a.n_points;
#pragma unroll
    for (int j = 0; j < OT; ++j) Av[j] = (rok && ook[j]) ? a.dz[row * a.ldz + a.zc0 + ocol[j]] : 0.0f;
#pragma unroll
    for (int j = 0; j < IT; ++j) Bv[j] = (rok && iok[j]) ? a.hin[row * a.ldh + a.hc0 + icol[j]] : 0.0f;
  };
#pragma unroll
  for (int k = 0; k < PF; ++k) load(s0 + k, A[k], B[k]);
  for (long long s = s0; s < s1; s += PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      float Ac[OT], Bc[IT];
#pragma unroll
      for (int j = 0; j < OT; ++j) Ac[j] = A[k][j];
#pragma unroll
      for (int j = 0; j < IT; ++j) Bc[j] = B[k][j];
      load(s + PF + k, A[k], B[k]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int jo = 0; jo < OT; ++jo) {
        bsum[jo] += Ac[jo];
#pragma unroll
        for (int ji = 0; ji < IT; ++ji) acc[jo][ji] = mfma32(Ac[jo], Bc[ji], acc[jo][ji]);
      }
    }
  }
  // D layout: column (lane&31) = in feature, row (r&3)+8(r>>2)+4h = out feature
#pragma unroll
  for (int jo = 0; jo < OT; ++jo)
#pragma unroll
    for (int ji = 0; ji < IT; ++ji) {
      const int cin = 32 * (wi * IT + ji) + i;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = 32 * (wo * OT + jo) + (r & 3) + 8 * (r >> 2) + 4 * h;
        if ((!NERF_WG_HACK_NOATOMIC || acc[jo][ji][r] == 1.2345678e33f) && rout < a.n_out && cin < a.n_in) atomicAdd(a.dw + (long long)rout * a.ldw + a.wc0 + cin, acc[jo][ji][r]);
      }
    }
  if (a.db != nullptr && wi == 0) {
#pragma unroll
    for (int j = 0; j < OT; ++j)
      if (ook[j]) atomicAdd(a.db + ocol[j], bsum[j]);
  }
}

// Fast path for the 256 x 256 layers (73 % of a training step before it existed).  Each lane loads
// ONE float4 per operand per k-step: lane i of a half reads columns 4i..4i+3 of its row, and element e
// of that float4 is the A (or B) operand of tile e -- i.e. the 128 columns of a wave are split into 4
// MFMA tiles with a stride-4 interleave (tile e = columns {4i+e}); the MFMA does not care which column
// a lane stands for, only the final scatter does.  2 x 16-B loads per 16 MFMAs, 4 k-steps in flight.
constexpr int kWgPf = 8;
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad256_f32_kernel(WgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wo = wave >> 1, wi = wave & 1;
  const long long n_pairs = (a.n_points + 1) / 2;
  const long long per = ((n_pairs + gridDim.x - 1) / gridDim.x + kWgPf - 1) / kWgPf * kWgPf;
  const long long s0 = (long long)blockIdx.x * per;
  long long s1 = s0 + per;
  if (s1 > n_pairs) s1 = n_pairs;
  const float* ap = a.dz + a.zc0 + 128 * wo + 4 * i;
  const float* bp = a.hin + a.hc0 + 128 * wi + 4 * i;

  f32x16 acc[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  f32x4 A[kWgPf], B[kWgPf];
  // unconditional loads (a predicated load makes the compiler wait for it on the spot): rows past the end read
  // the last row and are zeroed when consumed
  const long long last_row = a.n_points - 1;
  auto load = [&](long long s, f32x4& Av, f32x4& Bv) {
    long long row = 2 * s + h;
    row = row < last_row ? row : last_row;
    Av = *reinterpret_cast<const f32x4*>(ap + row * a.ldz);
    Bv = *reinterpret_cast<const f32x4*>(bp + row * a.ldh);
  };
#pragma unroll
  for (int k = 0; k < kWgPf; ++k) load(s0 + k, A[k], B[k]);
  for (long long s = s0; s < s1; s += kWgPf) {
#pragma unroll
    for (int k = 0; k < kWgPf; ++k) {
      const bool live = s + k < s1 && 2 * (s + k) + h < a.n_points;
      const f32x4 av = live ? A[k] : zero4, bv = live ? B[k] : zero4;
      load(s + kWgPf + k, A[k], B[k]);                 // refill this slot for kWgPf k-steps ahead
      __builtin_amdgcn_sched_barrier(0);
      bsum.x += av.x; bsum.y += av.y; bsum.z += av.z; bsum.w += av.w;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[e][f] = mfma32(av[e], bv[f], acc[e][f]);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int cin = 128 * wi + 4 * i + f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = 128 * wo + 4 * ((r & 3) + 8 * (r >> 2) + 4 * h) + e;
        if (!NERF_WG_HACK_NOATOMIC || acc[e][f][r] == 1.2345678e33f) atomicAdd(a.dw + (long long)rout * a.ldw + a.wc0 + cin, acc[e][f][r]);
      }
    }
  if (a.db != nullptr && wi == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicAdd(a.db + 128 * wo + 4 * i + e, bsum[e]);
  }
}

// The same 256 x 256 kernel with its operand ring filled by inline-asm loads (scalar row base + one lane offset, one
// s_waitcnt per k-step, no clamps or selects): with one wave per SIMD the ~230 VALU instructions per 128 MFMAs of
// the compiler-scheduled form were time off the matrix pipe.  The host only picks it when the point range splits into
// whole groups of 8 k-steps (16 points) per workgroup, so no row is ever out of range.  The asm loads complete behind
// the compiler's back (see nerf_mlp_f32.hip.inc): the consumed slot is refilled only after the 16 MFMAs that read it
// have been issued, and tools/check_asm_stream.py covers this kernel too.
// Several layers can share one launch ("jobs": blockIdx % n_jobs picks the layer, as in nerf_wgrad_bf16x3.hip.inc):
// a workgroup then integrates n_jobs times more points before its 65 536 atomic adds, and workgroups that finish
// together add to different matrices.
constexpr int kWgMaxJobs = 8;
struct WgradBatch {
  WgradArgs job[kWgMaxJobs];
  int n_jobs;
};
template <bool LIST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad256_f32_asm_kernel(WgradBatch batch) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 31, h = lane >> 5;
  const int wo = wave >> 1, wi = wave & 1;
  const int jid = blockIdx.x % batch.n_jobs, slice = blockIdx.x / batch.n_jobs, n_slices = gridDim.x / batch.n_jobs;
  if (slice >= n_slices) return;                                             // grid not a multiple of n_jobs
  const WgradArgs& a = batch.job[jid];
  // a group = 8 k-steps = 16 points; LIST: the groups are the halves of the live 32-point tiles, in list order
  const long long n_groups = LIST ? 2LL * *a.n_live : a.n_points / 16;        // host: n_points % 16 == 0 (LIST: % 32)
  const long long g0 = n_groups * slice / n_slices, g1 = n_groups * (slice + 1) / n_slices;
  if (g0 >= g1) return;
  const unsigned strideA = (unsigned)a.ldz * 8u, strideB = (unsigned)a.ldh * 8u;    // bytes per k-step (2 rows)
  auto group_kstep = [&](long long g) -> long long {                          // (uniform) first k-step of group g
    if (LIST) return 16LL * uniform_load_i32(a.live_tiles + (g >> 1)) + 8 * (g & 1);
    return 8 * g;
  };
  const char* abase = reinterpret_cast<const char*>(a.dz) + group_kstep(g0) * (long long)strideA;
  const char* bbase = reinterpret_cast<const char*>(a.hin) + group_kstep(g0) * (long long)strideB;
  const unsigned voffA = ((unsigned)h * (unsigned)a.ldz + (unsigned)(a.zc0 + 128 * wo + 4 * i)) * 4u;
  const unsigned voffB = ((unsigned)h * (unsigned)a.ldh + (unsigned)(a.hc0 + 128 * wi + 4 * i)) * 4u;

  f32x16 acc[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  f32x4 A[kWgPf], B[kWgPf];
#define NERF_WG_LD(dst, voff, base) asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst) : "v"(voff), "s"(base) : "memory")
#pragma unroll
  for (int k = 0; k < kWgPf; ++k) {
    NERF_WG_LD(A[k], voffA, abase + (long long)k * strideA);
    NERF_WG_LD(B[k], voffB, bbase + (long long)k * strideB);
  }
  const long long n_it = g1 - g0;
  for (long long it = 0; it < n_it; ++it) {
    // refill addresses: the next group of this workgroup, or -- in its last iteration -- the current rows again (a
    // branch-free way to stay inside the buffer; what those loads bring is never used)
    const long long ks = group_kstep(g0 + (it + 1 < n_it ? it + 1 : it));
    abase = reinterpret_cast<const char*>(a.dz) + ks * (long long)strideA;
    bbase = reinterpret_cast<const char*>(a.hin) + ks * (long long)strideB;
#pragma unroll
    for (int k = 0; k < kWgPf; ++k) {
      asm volatile("s_waitcnt vmcnt(14)" : "+v"(A[k]), "+v"(B[k]) :: "memory");   // all but the 14 newest loads have landed: slot k
      __builtin_amdgcn_sched_barrier(0);
      bsum.x += A[k].x; bsum.y += A[k].y; bsum.z += A[k].z; bsum.w += A[k].w;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[e][f] = mfma32(A[k][e], B[k][f], acc[e][f]);
      __builtin_amdgcn_sched_barrier(0);
      NERF_WG_LD(A[k], voffA, abase + (long long)k * strideA);
      NERF_WG_LD(B[k], voffB, bbase + (long long)k * strideB);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)"                      // drain the (unused) last refills before the registers are reused
               : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6]), "+v"(A[7]),
                 "+v"(B[0]), "+v"(B[1]), "+v"(B[2]), "+v"(B[3]), "+v"(B[4]), "+v"(B[5]), "+v"(B[6]), "+v"(B[7]) :: "memory");
#undef NERF_WG_LD
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int cin = 128 * wi + 4 * i + f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = 128 * wo + 4 * ((r & 3) + 8 * (r >> 2) + 4 * h) + e;
        if (!NERF_WG_HACK_NOATOMIC || acc[e][f][r] == 1.2345678e33f) atomicAdd(a.dw + (long long)rout * a.ldw + a.wc0 + cin, acc[e][f][r]);
      }
    }
  if (a.db != nullptr && wi == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicAdd(a.db + 128 * wo + 4 * i + e, bsum[e]);
  }
}

// Vector-load variant for the small layers (PE -> 256, views, alpha, rgb), which are HBM/latency bound:
// AV (BV) consecutive features per lane per row come in as one 4/8/16-byte load, feature AV*(32 wo + i) + e
// belongs to out-tile e (same for in-tiles), and kWgPf k-steps (16 points) are in flight per wave.
// Garbage in columns >= n_out / n_in (padding, or masked-off loads) only reaches outputs that are never written.
template <int N> struct WgVec;
template <> struct WgVec<1> { typedef float type; };
template <> struct WgVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct WgVec<4> { typedef float type __attribute__((ext_vector_type(4))); };
template <int N> __device__ __forceinline__ float wg_elem(const typename WgVec<N>::type& v, int e) { return v[e]; }
template <> __device__ __forceinline__ float wg_elem<1>(const float& v, int) { return v; }

constexpr int kWgVecPf = 8;
template <int AV, int BV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad_vec_f32_kernel(WgradArgs a) {
  typedef typename WgVec<AV>::type avec;
  typedef typename WgVec<BV>::type bvec;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wo = wave / a.isplit, wi = wave % a.isplit;
  const long long n_pairs = (a.n_points + 1) / 2;
  const long long per = ((n_pairs + gridDim.x - 1) / gridDim.x + kWgVecPf - 1) / kWgVecPf * kWgVecPf;
  const long long s0 = (long long)blockIdx.x * per;
  long long s1 = s0 + per;
  if (s1 > n_pairs) s1 = n_pairs;
  const int acol = AV * (32 * wo + i), bcol = BV * (32 * wi + i);
  const bool aok = acol + AV <= a.n_out || (AV == 1 && acol < a.n_out);         // whole vector readable
  const bool bok = a.hc0 + bcol + BV <= a.ldh;
  // loads are unconditional (a predicated load makes the compiler wait for it on the spot): out-of-range lanes
  // read column 0 / the last row instead and are zeroed when the value is consumed
  const float* ap = a.dz + a.zc0 + (aok ? acol : 0);
  const float* bp = a.hin + a.hc0 + (bok ? bcol : 0);
  const long long last_row = a.n_points - 1;

  f32x16 acc[AV][BV];
#pragma unroll
  for (int e = 0; e < AV; ++e)
#pragma unroll
    for (int f = 0; f < BV; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
  float bsum[AV];
#pragma unroll
  for (int e = 0; e < AV; ++e) bsum[e] = 0.0f;

  avec A[kWgVecPf];
  bvec B[kWgVecPf];
  auto load = [&](long long s, avec& Av, bvec& Bv) {
    long long row = 2 * s + h;
    row = row < last_row ? row : last_row;
    Av = *reinterpret_cast<const avec*>(ap + row * a.ldz);
    Bv = *reinterpret_cast<const bvec*>(bp + row * a.ldh);
  };
#pragma unroll
  for (int k = 0; k < kWgVecPf; ++k) load(s0 + k, A[k], B[k]);
  for (long long s = s0; s < s1; s += kWgVecPf) {
#pragma unroll
    for (int k = 0; k < kWgVecPf; ++k) {
      const bool live = s + k < s1 && 2 * (s + k) + h < a.n_points;
      const avec av = (live && aok) ? A[k] : avec(0.0f);
      const bvec bv = (live && bok) ? B[k] : bvec(0.0f);
      load(s + kWgVecPf + k, A[k], B[k]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        bsum[e] += wg_elem<AV>(av, e);
#pragma unroll
        for (int f = 0; f < BV; ++f) acc[e][f] = mfma32(wg_elem<AV>(av, e), wg_elem<BV>(bv, f), acc[e][f]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < AV; ++e)
#pragma unroll
    for (int f = 0; f < BV; ++f) {
      const int cin = bcol + f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = AV * (32 * wo + (r & 3) + 8 * (r >> 2) + 4 * h) + e;
        if (rout < a.n_out && cin < a.n_in) if (!NERF_WG_HACK_NOATOMIC || acc[e][f][r] == 1.2345678e33f) atomicAdd(a.dw + (long long)rout * a.ldw + a.wc0 + cin, acc[e][f][r]);
      }
    }
  if (a.db != nullptr && wi == 0) {
#pragma unroll
    for (int e = 0; e < AV; ++e)
      if (acol + e < a.n_out) atomicAdd(a.db + acol + e, bsum[e]);
  }
}

// The small-layer kernel on an inline-asm operand ring (what nerf_wgrad256_f32_asm_kernel is to nerf_wgrad256_f32_kernel):
// scalar row base + one lane offset per operand, one s_waitcnt per k-step, no clamps, selects or 64-bit lane address
// arithmetic -- the compiler-scheduled form spends ~30 VALU instructions per k-step on those, for only AV*BV MFMAs
// (1...8), and keeps 8 k-steps in flight; with one wave per SIMD that left the matrix pipe 23-53 % busy and the
// HBM-bound shapes (alpha_linear, rgb_linear, the direction part) at a third of the bandwidth.  PF k-steps (2 PF
// points) are in flight per wave, chosen per shape on the host: enough MFMA time (or bytes) to cover HBM latency.
// Host contract: n_points % (2 PF) == 0 and at least one group per workgroup, so no row is ever out of range; lanes
// whose columns do not exist read column 0 of their operand (finite or not: an MFMA row/column only ever reaches its
// own outputs, and those are never written).  tools/check_asm_stream.py covers every instance.
template <int N> struct WgAsmLd;
template <> struct WgAsmLd<1> {
  static __device__ __forceinline__ void ld(float& d, unsigned voff, const char* base) {
    asm volatile("global_load_dword %0, %1, %2" : "=&v"(d) : "v"(voff), "s"(base) : "memory");
  }
};
template <> struct WgAsmLd<2> {
  static __device__ __forceinline__ void ld(WgVec<2>::type& d, unsigned voff, const char* base) {
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(d) : "v"(voff), "s"(base) : "memory");
  }
};
template <> struct WgAsmLd<4> {
  static __device__ __forceinline__ void ld(WgVec<4>::type& d, unsigned voff, const char* base) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(d) : "v"(voff), "s"(base) : "memory");
  }
};

template <int AV, int BV, int PF, bool LIST = false>      // LIST: the groups are the live 32-point tiles (PF == 16: one tile per group)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad_vec_f32_asm_kernel(WgradArgs a) {
  static_assert(2 * PF - 2 <= 63, "vmcnt is a 6-bit counter");
  static_assert(!LIST || PF == 16, "a list entry is a 32-point tile = 16 k-steps");
  typedef typename WgVec<AV>::type avec;
  typedef typename WgVec<BV>::type bvec;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 31, h = lane >> 5;
  const int wo = wave / a.isplit, wi = wave % a.isplit;
  const long long n_groups = LIST ? (long long)*a.n_live : a.n_points / (2 * PF);      // host: n_points % (2 PF) == 0
  const long long g0 = n_groups * blockIdx.x / gridDim.x, g1 = n_groups * (blockIdx.x + 1) / gridDim.x;
  if (g0 >= g1) return;
  const unsigned strideA = (unsigned)a.ldz * 8u, strideB = (unsigned)a.ldh * 8u;    // bytes per k-step (2 rows)
  auto group_kstep = [&](long long g) -> long long { return (long long)PF * (LIST ? (long long)uniform_load_i32(a.live_tiles + g) : g); };   // (uniform)
  const char* abase = reinterpret_cast<const char*>(a.dz) + group_kstep(g0) * (long long)strideA;
  const char* bbase = reinterpret_cast<const char*>(a.hin) + group_kstep(g0) * (long long)strideB;
  const int acol = AV * (32 * wo + i), bcol = BV * (32 * wi + i);
  const bool aok = acol + AV <= a.n_out || (AV == 1 && acol < a.n_out);
  const bool bok = a.hc0 + bcol + BV <= a.ldh;
  const unsigned voffA = ((unsigned)h * (unsigned)a.ldz + (unsigned)(a.zc0 + (aok ? acol : 0))) * 4u;
  const unsigned voffB = ((unsigned)h * (unsigned)a.ldh + (unsigned)(a.hc0 + (bok ? bcol : 0))) * 4u;

  f32x16 acc[AV][BV];
#pragma unroll
  for (int e = 0; e < AV; ++e)
#pragma unroll
    for (int f = 0; f < BV; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
  float bsum[AV];
#pragma unroll
  for (int e = 0; e < AV; ++e) bsum[e] = 0.0f;

  avec A[PF];
  bvec B[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    WgAsmLd<AV>::ld(A[k], voffA, abase + (long long)k * strideA);
    WgAsmLd<BV>::ld(B[k], voffB, bbase + (long long)k * strideB);
  }
  const long long n_it = g1 - g0;
  for (long long it = 0; it < n_it; ++it) {
    // refill addresses: the next group, or -- in the last iteration -- the current rows again (never used)
    const long long ks = group_kstep(g0 + (it + 1 < n_it ? it + 1 : it));
    abase = reinterpret_cast<const char*>(a.dz) + ks * (long long)strideA;
    bbase = reinterpret_cast<const char*>(a.hin) + ks * (long long)strideB;
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      asm volatile("s_waitcnt vmcnt(%2)" : "+v"(A[k]), "+v"(B[k]) : "n"(2 * PF - 2) : "memory");   // slot k has landed
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        bsum[e] += wg_elem<AV>(A[k], e);
#pragma unroll
        for (int f = 0; f < BV; ++f) acc[e][f] = mfma32(wg_elem<AV>(A[k], e), wg_elem<BV>(B[k], f), acc[e][f]);
      }
      __builtin_amdgcn_sched_barrier(0);
      WgAsmLd<AV>::ld(A[k], voffA, abase + (long long)k * strideA);
      WgAsmLd<BV>::ld(B[k], voffB, bbase + (long long)k * strideB);
    }
  }
#pragma unroll
  for (int k = 0; k < PF; ++k)                                 // drain the (unused) last refills before the registers are reused
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(A[k]), "+v"(B[k]) :: "memory");
#pragma unroll
  for (int e = 0; e < AV; ++e)
#pragma unroll
    for (int f = 0; f < BV; ++f) {
      const int cin = bcol + f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = AV * (32 * wo + (r & 3) + 8 * (r >> 2) + 4 * h) + e;
        if (rout < a.n_out && cin < a.n_in) if (!NERF_WG_HACK_NOATOMIC || acc[e][f][r] == 1.2345678e33f) atomicAdd(a.dw + (long long)rout * a.ldw + a.wc0 + cin, acc[e][f][r]);
      }
    }
  if (a.db != nullptr && wi == 0) {
#pragma unroll
    for (int e = 0; e < AV; ++e)
      if (acol + e < a.n_out) atomicAdd(a.db + acol + e, bsum[e]);
  }
}
