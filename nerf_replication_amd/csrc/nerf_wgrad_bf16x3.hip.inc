// Weight-gradient GEMM of the 256 x 256 layers on the bf16 matrix cores with three-way split operands
// (fp32-accurate: v = hi + mid + lo, 8 mantissa bits each, exact truncation splits; the six products down
// to 2^-16 are kept.  The three dropped ones, mid lo + lo mid + lo lo, are below 2^-24 of the term only for typical
// operands (median 2^-25); they reach 2^-21 of it for significands 1.0000000 followed by ones, and are bounded by
// (2^-20 + 2^-27) of it: |mid| < 2^-7 |v|, |lo| < 2^-14 |v|.  tests/test_wgrad_reference_cpu.py holds these figures.)
//
//   dW[o][i] += sum_p dZ[p][o] * Hin[p][i]        (autograd of nn.Linear, network.py:22-47)
//
// Why bf16 and not the fp16 hi/lo split of the MLP chains: the reduction index is the point, so a per-point
// scale cannot be factored out, and gradients (1e-6 .. 1e-8 with a mean-reduced loss) are far outside the
// fp16 range.  bf16 has the fp32 exponent, so no scaling and no statistics pass are needed.  Per 16 points
// a wave issues 6 x 16 v_mfma_f32_32x32x16_bf16 (3072 cycles) against 16 x 8 fp32 MFMAs (8192 cycles) of
// nerf_wgrad256_f32_asm_kernel.  All 256 x 256 layers of one sub-network are one launch ("jobs": blockIdx % n_jobs),
// so a workgroup integrates 8x more points before its 65536 atomic adds and concurrently running workgroups
// add to different matrices.
#include "nerf_mlp_common.h"

struct WgradXJob {
  const float* dz; const float* hin; float* dw; float* db;
  int ldz, zc0, ldh, hc0, ldw, wc0;
};
constexpr int kWgxMaxJobs = 8;
struct WgradXArgs {
  WgradXJob job[kWgxMaxJobs];
  int n_jobs;
  long long n_points;
  // optional live-tile list of the backward pass (nerf_tile_flags_kernel / nerf_tile_scan_kernel; n_points % 32 == 0): the
  // 16-point steps are then the halves of the live 32-point tiles, in list order; dead tiles' rows are never read
  const int* live_tiles;
  const int* n_live;
};

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// eight points of one feature -> packed (hi, mid, lo) bf16 fragments; every residual is exact
__device__ __forceinline__ void split3_bf16(const float (&v)[8], u32x4& H, u32x4& M, u32x4& L) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned hb[2], mb[2], lb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float x = v[2 * q + k];
      hb[k] = __float_as_uint(x) & 0xffff0000u;
      const float r1 = x - __uint_as_float(hb[k]);
      mb[k] = __float_as_uint(r1) & 0xffff0000u;
      const float r2 = r1 - __uint_as_float(mb[k]);
      lb[k] = __float_as_uint(r2);
    }
    H[q] = __builtin_amdgcn_perm(hb[1], hb[0], 0x07060302u);      // {odd point : even point} upper halves
    M[q] = __builtin_amdgcn_perm(mb[1], mb[0], 0x07060302u);
    L[q] = __builtin_amdgcn_perm(lb[1], lb[0], 0x07060302u);
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_wgrad256_bf16x3_kernel(WgradXArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 31, g = lane >> 5;
  const int wo = wave >> 1, wi = wave & 1;
  const int jid = blockIdx.x % a.n_jobs, slice = blockIdx.x / a.n_jobs, n_slices = gridDim.x / a.n_jobs;
  if (slice >= n_slices) return;                                  // grid not a multiple of n_jobs
  const WgradXJob& J = a.job[jid];
  const bool list = a.live_tiles != nullptr;                        // (uniform)
  const long long n_steps = list ? 2LL * *a.n_live : (a.n_points + 15) / 16;
  const long long per = (n_steps + n_slices - 1) / n_slices;
  const long long s0 = (long long)slice * per;
  long long s1 = s0 + per;
  if (s1 > n_steps) s1 = n_steps;
  if (s0 >= s1) return;                                           // (uniform) nothing in this slice

  // Operand rows travel HBM -> LDS by DMA three steps ahead of their use (no registers held while in flight,
  // 96 KB per CU in flight: with register prefetch of one step the kernel ran at 2.7 TB/s, latency-bound), and
  // every row is fetched once per workgroup instead of once per wave pair.  A step's stage is 32 KB: 16 rows of
  // dZ (1 KiB each: ld = 256 floats, column 0, checked by the host) then 16 rows of Hin.  Wave w owns rows
  // 4w..4w+3 of both.  Timeline of step s:  DMA(s+3) is issued;  registers already hold raw(s) (read from LDS
  // during step s-1);  split(s);  ds_read raw(s+1) (certified at the end of step s-1);  96 MFMAs;
  // s_waitcnt vmcnt(8) (only DMA(s+3) may be outstanding: stage s+2 has landed) + s_barrier (everyone's part of
  // s+2 has landed, everyone has read s+1's predecessor).  The stage DMA(s+3) overwrites held step s-1, whose
  // reads finished two barriers ago.
  constexpr int kStageBytes = 32768, kStages = 4;
  __shared__ __attribute__((aligned(16))) char stage_generic[kStages * kStageBytes];
  lds_char* stage0 = (lds_char*)stage_generic;
  const char* abase = reinterpret_cast<const char*>(J.dz);
  const char* bbase = reinterpret_cast<const char*>(J.hin);
  const long long last_row = a.n_points - 1;
  auto dma = [&](long long s) {                                   // this wave's 8 rows of step s -> stage s % 4
    lds_char* dst = stage0 + (int)((s - s0) & (kStages - 1)) * kStageBytes + (4 * wave) * 1024;
    long long row0 = 16 * s;                                      // (uniform) first point of step s
    if (list) {                                                   // steps past the slice re-read its last step (never used)
      const long long sc = s < s1 ? s : s1 - 1;
      row0 = 32LL * uniform_load_i32(a.live_tiles + (sc >> 1)) + 16 * (sc & 1);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      long long row = row0 + 4 * wave + k;
      row = row < last_row ? row : last_row;                      // past the end: re-read the last row (zeroed on use)
      // (uniform 64-bit row address + 32-bit lane offset: the address stays in SGPRs)
      __builtin_amdgcn_global_load_lds((gbl_void*)((abase + row * 1024) + (unsigned)lane * 16u), (lds_void*)(dst + k * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void*)((bbase + row * 1024) + (unsigned)lane * 16u), (lds_void*)(dst + 16384 + k * 1024), 16, 0, 0);
    }
  };
  // the same, one row pair (k = 0..3) at a time: the steady-state loop issues the 8 pieces of a step between its MFMAs (each costs
  // 60-180 cycles of issue beside other memory work -- MI355X_MICROARCH.md -- which a burst in front of the MFMAs left exposed)
  // (uniform) first point of step s.  List mode: the tile index comes from memory -- fetched ONE STEP AHEAD of its use (tl_next):
  // looked up where it is needed, the scalar load's latency (and the lgkmcnt(0) wait hipcc puts in front of its use) was exposed
  // in every step: 400-800 of a step's ~5000 cycles (s_memtime stamps, LAB_NOTEBOOK.md A9)
  auto live_tile_of = [&](long long s) -> int { const long long sc = s < s1 ? s : s1 - 1; return uniform_load_i32(a.live_tiles + (sc >> 1)); };
  auto dma_row0 = [&](long long s, int tl) -> long long {
    if (!list) return 16 * s;
    const long long sc = s < s1 ? s : s1 - 1;
    return 32LL * tl + 16 * (sc & 1);
  };
  auto dma_piece = [&](long long s, long long row0, int k) {
    lds_char* dst = stage0 + (int)((s - s0) & (kStages - 1)) * kStageBytes + (4 * wave) * 1024;
    long long row = row0 + 4 * wave + k;
    row = row < last_row ? row : last_row;
    __builtin_amdgcn_global_load_lds((gbl_void*)((abase + row * 1024) + (unsigned)lane * 16u), (lds_void*)(dst + k * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void*)((bbase + row * 1024) + (unsigned)lane * 16u), (lds_void*)(dst + 16384 + k * 1024), 16, 0, 0);
  };
  // this lane's LDS byte offset inside a stage: row 8g (+ j), columns 128 wo + 4 i .. +3 (A) / 128 wi + 4 i (B, + 16 KiB)
  const unsigned la = (unsigned)(8 * g) * 1024u + (unsigned)(128 * wo + 4 * i) * 4u;
  const unsigned lb = (unsigned)(8 * g) * 1024u + (unsigned)(128 * wi + 4 * i) * 4u + 16384u;

  f32x16 acc[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][f][r] = 0.0f;
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  f32x4 RA[8], RB[8];
  // LDS -> registers with inline asm (a plain load whose first use is in the next iteration gets sunk to that use)
  auto lds_read = [&](long long s) {
    const unsigned sb = (unsigned)(size_t)stage0 + (unsigned)((s - s0) & (kStages - 1)) * (unsigned)kStageBytes;
    const unsigned pa = sb + la, pb = sb + lb;
#define NERF_WGX_DS(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:" #imm : "=&v"(dst) : "v"(addr) : "memory")
    NERF_WGX_DS(RA[0], pa, 0);    NERF_WGX_DS(RB[0], pb, 0);
    NERF_WGX_DS(RA[1], pa, 1024); NERF_WGX_DS(RB[1], pb, 1024);
    NERF_WGX_DS(RA[2], pa, 2048); NERF_WGX_DS(RB[2], pb, 2048);
    NERF_WGX_DS(RA[3], pa, 3072); NERF_WGX_DS(RB[3], pb, 3072);
    NERF_WGX_DS(RA[4], pa, 4096); NERF_WGX_DS(RB[4], pb, 4096);
    NERF_WGX_DS(RA[5], pa, 5120); NERF_WGX_DS(RB[5], pb, 5120);
    NERF_WGX_DS(RA[6], pa, 6144); NERF_WGX_DS(RB[6], pb, 6144);
    NERF_WGX_DS(RA[7], pa, 7168); NERF_WGX_DS(RB[7], pb, 7168);
#undef NERF_WGX_DS
  };
  dma(s0); dma(s0 + 1); dma(s0 + 2);
  asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");      // stages s0 and s0+1 landed, for every wave
  __builtin_amdgcn_sched_barrier(0);
  lds_read(s0);
  int tl_cur = list ? live_tile_of(s0 + 3) : 0, tl_next = list ? live_tile_of(s0 + 4) : 0;      // tiles of steps s + 3, s + 4
  for (long long s = s0; s < s1; ++s) {
    __builtin_amdgcn_sched_barrier(0);
    const long long r3 = dma_row0(s + 3, tl_cur);
    tl_cur = tl_next;
    __builtin_amdgcn_sched_barrier(0);
    // the asm LDS reads are invisible to the compiler's own waitcnt bookkeeping
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(RA[0]), "+v"(RA[1]), "+v"(RA[2]), "+v"(RA[3]), "+v"(RA[4]), "+v"(RA[5]), "+v"(RA[6]), "+v"(RA[7]),
                   "+v"(RB[0]), "+v"(RB[1]), "+v"(RB[2]), "+v"(RB[3]), "+v"(RB[4]), "+v"(RB[5]), "+v"(RB[6]), "+v"(RB[7])
                 :: "memory");
    if (!list && 16 * s + 16 > a.n_points) {                       // ragged last step (uniform branch): rows past the end count as zero
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (16 * s + 8 * g + j >= a.n_points) { RA[j] = zero4; RB[j] = zero4; }
    }
    // The dZ side is split one feature group `e` at a time, group e + 1 behind the 24 MFMAs of group e (round 3: all 64 values
    // were split in front of the 96 MFMAs, ~350 VALU with the matrix pipe idle -- one wave per SIMD -- and MFMA busy was 0.36);
    // only the Hin side (needed by every group) and group 0 are split up front.  Every accumulator still receives its six terms
    // in the same order (smallest first), so the result is bit-identical.
    u32x4 BH[4], BM[4], BL[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      float vb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) vb[j] = RB[j][f];
      split3_bf16(vb, BH[f], BM[f], BL[f]);
    }
    u32x4 AH0, AM0, AL0, AH1, AM1, AL1;
#define NERF_WGX_SPLIT_A(E, H, M, L) do {                                                           \
      float va[8];                                                                                 \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) va[j] = RA[j][E];                               \
      bsum[E] += ((va[0] + va[1]) + (va[2] + va[3])) + ((va[4] + va[5]) + (va[6] + va[7]));        \
      split3_bf16(va, H, M, L);                                                                    \
    } while (0)
    // smallest terms first; 4 independent accumulators between two uses of the same one
#define NERF_WGX_TERM(E, AX, BX) _Pragma("unroll") for (int f = 0; f < 4; ++f) acc[E][f] = mfma_bf16(AX, BX[f], acc[E][f]);
#define NERF_WGX_GROUP(E, H, M, L)                                                                  \
      NERF_WGX_TERM(E, L, BH) NERF_WGX_TERM(E, H, BL) NERF_WGX_TERM(E, M, BM)                       \
      NERF_WGX_TERM(E, M, BH) NERF_WGX_TERM(E, H, BM) NERF_WGX_TERM(E, H, BH)                       \
      _Pragma("unroll") for (int k = 0; k < 24; ++k) {      /* one MFMA, then up to three of the next group's split instructions */ \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                          \
        if (k == 7 || k == 15) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   /* ... and this group's two DMA instructions */ \
      }
    NERF_WGX_SPLIT_A(0, AH0, AM0, AL0);
    __builtin_amdgcn_sched_barrier(0);
    // the next tile index: requested HERE, behind this step's lgkmcnt(0) wait (a scalar load counts on lgkmcnt too: issued in front
    // of that wait, its whole latency was exposed in every step), consumed at the top of the next step
    if (list) tl_next = live_tile_of(s + 5);
    __builtin_amdgcn_sched_barrier(0);
    NERF_WGX_SPLIT_A(1, AH1, AM1, AL1); dma_piece(s + 3, r3, 0);
    NERF_WGX_GROUP(0, AH0, AM0, AL0)
    __builtin_amdgcn_sched_barrier(0);
    NERF_WGX_SPLIT_A(2, AH0, AM0, AL0); dma_piece(s + 3, r3, 1);
    NERF_WGX_GROUP(1, AH1, AM1, AL1)
    __builtin_amdgcn_sched_barrier(0);
    NERF_WGX_SPLIT_A(3, AH1, AM1, AL1); dma_piece(s + 3, r3, 2);
    NERF_WGX_GROUP(2, AH0, AM0, AL0)
    __builtin_amdgcn_sched_barrier(0);
    lds_read(s + 1);                               // RA / RB are consumed; lands during the 24 MFMAs below (past the slice: the re-read last step, never used)
    __builtin_amdgcn_sched_barrier(0);
    dma_piece(s + 3, r3, 3);
    NERF_WGX_GROUP(3, AH1, AM1, AL1)
#undef NERF_WGX_GROUP
#undef NERF_WGX_TERM
#undef NERF_WGX_SPLIT_A
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");    // stage s+2 landed everywhere; stage s+1 fully read
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       // no DMA (or read of the step past the slice) may be in flight when the LDS is released
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int cin = 128 * wi + 4 * i + f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rout = 128 * wo + 4 * ((r & 3) + 8 * (r >> 2) + 4 * g) + e;
        atomicAdd(J.dw + (long long)rout * J.ldw + J.wc0 + cin, acc[e][f][r]);
      }
    }
  if (J.db != nullptr && wi == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = bsum[e] + __shfl_xor(bsum[e], 32);
      if (g == 0) atomicAdd(J.db + 128 * wo + 4 * i + e, t);
    }
  }
}
