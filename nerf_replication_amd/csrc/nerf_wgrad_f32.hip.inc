#ifndef NERF_WG_HACK_NOATOMIC         // timing-only: the weight-gradient kernels drop their final atomic adds (wrong results)
#define NERF_WG_HACK_NOATOMIC 0
#endif
// Weight-gradient GEMM for the training path (fp32 MFMA): dW[o][i] += sum_p dZ[p][o] * Hin[p][i].
// (csrc/nerf_wgrad_table.h says which instance serves which shape)
//
// This is what autograd computes for every nn.Linear of network.py:22-47 (grad_weight = grad_out^T @
// input, grad_bias = grad_out.sum(0)).  The reduction index is the POINT, so both MFMA operands want
// "feature on the lane, point on k": exactly what row-major [P, C] activations give (lanes 0-31 read
// 128 contiguous bytes of row 2s, lanes 32-63 of row 2s+1).  Workgroups are persistent over
// contiguous point ranges, each wave keeps OT x IT 32x32 output tiles in registers (4x4 = 256
// accumulators for a 256x256 layer split over the 4 waves) and adds them to dW with float atomics
// at the end (256-B row segments per wave-instruction, the full-rate shape).
#include "nerf_mlp_common.h"

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

// Column of element t of lane column x in wave part w, for a wave that holds V tiles on that side.  The generic kernel
// keeps its tiles contiguous (tile t = columns 32t..32t+31 of the wave's part); the vector-load kernels read V consecutive
// floats per lane and give float t to tile t (tile t = columns {V x + t}): the MFMA does not care which column a lane
// stands for, only the loads and the final scatter do.
template <int V, bool INTERLEAVED>
__device__ __forceinline__ int wg_col(int w, int x, int t) { return INTERLEAVED ? V * (32 * w + x) + t : 32 * (w * V + t) + x; }

template <int OT, int IT>
__device__ __forceinline__ void wg_clear(f32x16 (&acc)[OT][IT], float (&bsum)[OT]) {
#pragma unroll
  for (int e = 0; e < OT; ++e) {
    bsum[e] = 0.0f;
#pragma unroll
    for (int f = 0; f < IT; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
  }
}

// The end of every kernel: a wave's tiles into dW, and (waves of the first in part) the column sums of dZ into db.
// D layout: column (lane&31) = in feature, row (r&3)+8(r>>2)+4h = out feature.  FULL: the instance is known to cover its
// shape exactly, no bounds tests.
template <int OT, int IT, bool INTERLEAVED, bool FULL>
__device__ __forceinline__ void wg_scatter(const WgradArgs& a, const f32x16 (&acc)[OT][IT], const float (&bsum)[OT], int wo, int wi,
                                           int i, int h) {
#pragma unroll
  for (int e = 0; e < OT; ++e)
#pragma unroll
    for (int f = 0; f < IT; ++f) {
      const int cin = wg_col<IT, INTERLEAVED>(wi, i, f);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = wg_col<OT, INTERLEAVED>(wo, (r & 3) + 8 * (r >> 2) + 4 * h, e);
        if (FULL || (rout < a.n_out && cin < a.n_in)) if (!NERF_WG_HACK_NOATOMIC || acc[e][f][r] == 1.2345678e33f) atomicAdd(a.dw + (long long)rout * a.ldw + a.wc0 + cin, acc[e][f][r]);
      }
    }
  if (a.db != nullptr && wi == 0) {
#pragma unroll
    for (int e = 0; e < OT; ++e) {
      const int ocol = wg_col<OT, INTERLEAVED>(wo, i, e);
      if (FULL || ocol < a.n_out) atomicAdd(a.db + ocol, bsum[e]);
    }
  }
}

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
  for (int j = 0; j < OT; ++j) { ocol[j] = wg_col<OT, false>(wo, i, j); ook[j] = ocol[j] < a.n_out; }
#pragma unroll
  for (int j = 0; j < IT; ++j) { icol[j] = wg_col<IT, false>(wi, i, j); iok[j] = icol[j] < a.n_in; }

  f32x16 acc[OT][IT];
  float bsum[OT];
  wg_clear(acc, bsum);

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
  wg_scatter<OT, IT, false, false>(a, acc, bsum, wo, wi, i, h);
}

// Vector-load kernel: AV (BV) consecutive features per lane per row come in as one 4/8/16-byte load, feature
// AV*(32 wo + i) + e belongs to out-tile e (same for in-tiles), and kWgPf k-steps (16 points) are in flight per wave.
// <4,4> split (2, 2) is the 256 x 256 layer (2 x 16-B loads per 16 MFMAs); the others serve the small layers (PE -> 256,
// views, alpha, rgb), which are HBM/latency bound.
// Garbage in columns >= n_out / n_in (padding, or masked-off loads) only reaches outputs that are never written.
template <int N> struct WgVec;
template <> struct WgVec<1> { typedef float type; };
template <> struct WgVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct WgVec<4> { typedef float type __attribute__((ext_vector_type(4))); };
template <int N> __device__ __forceinline__ float wg_elem(const typename WgVec<N>::type& v, int e) { return v[e]; }
template <> __device__ __forceinline__ float wg_elem<1>(const float& v, int) { return v; }

constexpr int kWgPf = 8;
template <int AV, int BV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad_vec_f32_kernel(WgradArgs a) {
  typedef typename WgVec<AV>::type avec;
  typedef typename WgVec<BV>::type bvec;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wo = wave / a.isplit, wi = wave % a.isplit;
  const long long n_pairs = (a.n_points + 1) / 2;
  const long long per = ((n_pairs + gridDim.x - 1) / gridDim.x + kWgPf - 1) / kWgPf * kWgPf;
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
  float bsum[AV];
  wg_clear(acc, bsum);

  avec A[kWgPf];
  bvec B[kWgPf];
  auto load = [&](long long s, avec& Av, bvec& Bv) {
    long long row = 2 * s + h;
    row = row < last_row ? row : last_row;
    Av = *reinterpret_cast<const avec*>(ap + row * a.ldz);
    Bv = *reinterpret_cast<const bvec*>(bp + row * a.ldh);
  };
#pragma unroll
  for (int k = 0; k < kWgPf; ++k) load(s0 + k, A[k], B[k]);
  for (long long s = s0; s < s1; s += kWgPf) {
#pragma unroll
    for (int k = 0; k < kWgPf; ++k) {
      const bool live = s + k < s1 && 2 * (s + k) + h < a.n_points;
      const avec av = (live && aok) ? A[k] : avec(0.0f);
      const bvec bv = (live && bok) ? B[k] : bvec(0.0f);
      load(s + kWgPf + k, A[k], B[k]);                 // refill this slot for kWgPf k-steps ahead
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        bsum[e] += wg_elem<AV>(av, e);
#pragma unroll
        for (int f = 0; f < BV; ++f) acc[e][f] = mfma32(wg_elem<AV>(av, e), wg_elem<BV>(bv, f), acc[e][f]);
      }
    }
  }
  wg_scatter<AV, BV, true, false>(a, acc, bsum, wo, wi, i, h);
}

// The vector-load kernel on an inline-asm operand ring: scalar row base + one lane offset per operand, one s_waitcnt per
// k-step, no clamps, selects or 64-bit lane address arithmetic.  The compiler-scheduled form spends ~30 VALU instructions
// per k-step on those (~230 per 128 MFMAs for <4,4>) and, with one wave per SIMD, that is time off the matrix pipe: it left
// the pipe 23-53 % busy on the small layers and the HBM-bound shapes (alpha_linear, rgb_linear, the direction part) at a
// third of the bandwidth.  PF k-steps (2 PF points) are in flight per wave, chosen per shape on the host: enough MFMA time
// (or bytes) to cover HBM latency.  The asm loads complete behind the compiler's back (see nerf_mlp_f32.hip.inc): a consumed
// slot is refilled only after the MFMAs that read it have been issued, and tools/check_asm_stream.py covers every instance.
//
// HOST CONTRACT -- nothing in the ring clamps, so these five rules are what keeps its loads inside the buffers:
//   1. the point range is whole groups of 2 PF points: n_points % (2 PF) == 0 (LIST: whole 32-point tiles, % 32);
//   2. a workgroup that does not exit has at least one group (a workgroup without one exits before its first load);
//   3. byte strides fit 32 bits: ld < 2^28 (the 256 x 256 launch asks ld * 8 < 2^31, the bytes of one k-step);
//   4. lanes whose columns do not exist read column 0 of their operand (finite or not: an MFMA row/column only ever
//      reaches its own outputs, and those are never written);
//   5. no load beyond the last row: the refill of a workgroup's last group reads that group again, and brings nothing used.
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

// One workgroup's share (slice of n_slices) of one job, start to end.  A group is PF k-steps; LIST: the groups are the
// 16 / PF parts of the live 32-point tiles, in list order.  FULL: the job is exactly 32 AV osplit x 32 BV isplit.
template <int AV, int BV, int PF, bool LIST, bool FULL>
__device__ __forceinline__ void wg_ring_job(const WgradArgs& a, int slice, int n_slices, int wo, int wi) {
  static_assert(2 * PF - 2 <= 63, "vmcnt is a 6-bit counter");
  static_assert(16 % PF == 0, "a list entry is a 32-point tile = 16 k-steps");
  typedef typename WgVec<AV>::type avec;
  typedef typename WgVec<BV>::type bvec;
  constexpr int GPT = 16 / PF;                                                // groups per live tile
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const long long n_groups = LIST ? (long long)GPT * *a.n_live : a.n_points / (2 * PF);
  const long long g0 = n_groups * slice / n_slices, g1 = n_groups * (slice + 1) / n_slices;
  if (g0 >= g1) return;
  const unsigned strideA = (unsigned)a.ldz * 8u, strideB = (unsigned)a.ldh * 8u;    // bytes per k-step (2 rows)
  auto group_kstep = [&](unsigned long long g) -> long long {                 // (uniform) first k-step of group g
    if (LIST) return 16LL * uniform_load_i32(a.live_tiles + g / GPT) + PF * (int)(g % GPT);
    return PF * (long long)g;
  };
  const char* abase = reinterpret_cast<const char*>(a.dz) + group_kstep(g0) * (long long)strideA;
  const char* bbase = reinterpret_cast<const char*>(a.hin) + group_kstep(g0) * (long long)strideB;
  const int acol = AV * (32 * wo + i), bcol = BV * (32 * wi + i);
  const bool aok = FULL || acol + AV <= a.n_out || (AV == 1 && acol < a.n_out);
  const bool bok = FULL || a.hc0 + bcol + BV <= a.ldh;
  const unsigned voffA = ((unsigned)h * (unsigned)a.ldz + (unsigned)(a.zc0 + (aok ? acol : 0))) * 4u;
  const unsigned voffB = ((unsigned)h * (unsigned)a.ldh + (unsigned)(a.hc0 + (bok ? bcol : 0))) * 4u;

  f32x16 acc[AV][BV];
  float bsum[AV];
  wg_clear(acc, bsum);

  avec A[PF];
  bvec B[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    WgAsmLd<AV>::ld(A[k], voffA, abase + (long long)k * strideA);
    WgAsmLd<BV>::ld(B[k], voffB, bbase + (long long)k * strideB);
  }
  const long long n_it = g1 - g0;
  for (long long it = 0; it < n_it; ++it) {
    // refill addresses: the next group of this workgroup, or -- in its last iteration -- the current rows again (a
    // branch-free way to stay inside the buffer; what those loads bring is never used)
    const long long ks = group_kstep(g0 + (it + 1 < n_it ? it + 1 : it));
    abase = reinterpret_cast<const char*>(a.dz) + ks * (long long)strideA;
    bbase = reinterpret_cast<const char*>(a.hin) + ks * (long long)strideB;
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      asm volatile("s_waitcnt vmcnt(%2)" : "+v"(A[k]), "+v"(B[k]) : "n"(2 * PF - 2) : "memory");   // all but the 2 PF - 2 newest loads have landed: slot k
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
  // drain the (unused) last refills before the registers are reused: in one statement where its 2 PF operands fit one
  if constexpr (PF == 8) {
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6]), "+v"(A[7]),
                   "+v"(B[0]), "+v"(B[1]), "+v"(B[2]), "+v"(B[3]), "+v"(B[4]), "+v"(B[5]), "+v"(B[6]), "+v"(B[7]) :: "memory");
  } else {
#pragma unroll
    for (int k = 0; k < PF; ++k) asm volatile("s_waitcnt vmcnt(0)" : "+v"(A[k]), "+v"(B[k]) :: "memory");
  }
  wg_scatter<AV, BV, true, FULL>(a, acc, bsum, wo, wi, i, h);
}

template <int AV, int BV, int PF, bool LIST = false>      // LIST: the groups are the live 32-point tiles (PF == 16: one tile per group)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad_vec_f32_asm_kernel(WgradArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  wg_ring_job<AV, BV, PF, LIST, false>(a, blockIdx.x, gridDim.x, wave / a.isplit, wave % a.isplit);
}

// The 256 x 256 layers on the ring: <4,4>, waves split (2, 2), groups of kWgPf k-steps (16 points; LIST: the halves of the
// live tiles), and no bounds test anywhere.  Several layers can share one launch ("jobs": blockIdx % n_jobs picks the layer,
// as in nerf_wgrad_bf16x3.hip.inc): a workgroup then integrates n_jobs times more points before its 65 536 atomic adds, and
// workgroups that finish together add to different matrices.  (73 % of a training step went to these layers before a
// kernel of their own existed.)
constexpr int kWgMaxJobs = 8;
struct WgradBatch {
  WgradArgs job[kWgMaxJobs];
  int n_jobs;
};
template <bool LIST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad256_f32_asm_kernel(WgradBatch batch) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int jid = blockIdx.x % batch.n_jobs, slice = blockIdx.x / batch.n_jobs, n_slices = gridDim.x / batch.n_jobs;
  if (slice >= n_slices) return;                                             // grid not a multiple of n_jobs
  wg_ring_job<4, 4, kWgPf, LIST, true>(batch.job[jid], slice, n_slices, wave >> 1, wave & 1);
}
