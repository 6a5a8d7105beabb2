// Fused positional-encoding + 8+1-layer NeRF MLP, exact fp32 on v_mfma_f32_32x32x2_f32.
//
// Replaces, per 32-point tile, the reference's
//   Network.forward   src/models/nerf/network.py:199-258   (PE + batchify(512) loop)
//   Encoder.embed     src/models/encoding/freq.py:31-32
//   NeRF.forward      src/models/nerf/network.py:49-74     (12 nn.Linear + 3 cat per chunk)
// and, in ray mode, the point construction of volume_renderer.py:63 / :267 and viewdirs :314.
//
// One wavefront owns 32 points for the whole network.  Activations never leave registers:
// the accumulator tile of layer l IS the B operand of layer l+1 (see nerf_layout.h), the two
// 128-register activation sets X/Y ping-pong, and the only memory stream is the pre-permuted
// weights (1 KiB per 4 MFMAs per wave, L2-resident: 2.39 MB per model).
// Measured anatomy (tools/ab_bench.py, timing-only NERF_F32_HACK_* variants, 155.4 TFLOP/s raw MFMA
// rate from tools/micro/mfma_f32_rate.hip): weight loads cost 7.8 % whatever the prefetch distance
// (3..15 blocks identical: not latency), bias loads 1.7 %, ReLU + AGPR moves 1.3 %, sincos 0.6 %;
// with all of them removed the same MFMA stream runs at 150 TFLOP/s.
//   registers: 128 (X) + 128 (Y) + 32 (xyz PE, kept for the skip) + 16 (dir PE) + prefetch
//   -> 1 wave per SIMD with the full 512-entry VGPR+AGPR file; MFMA-bound by construction:
//   8256 MFMAs x 64 cycles per tile vs ~1.5k VALU instructions (9280 before feature_linear was folded into the views
//   layer, nerf_layout.h kFold*; the training forward still issues 9280: it keeps the feature GEMM for the backward pass).

#include "nerf_mlp_common.h"

// timing-only diagnostics for tools/ab_bench.py (never set in the shipped build: they break numerics)
#ifndef NERF_F32_WG_WAVES
#define NERF_F32_WG_WAVES 1                 // waves per workgroup of the (barrier-free) inference instance: with one-wave
                                            // workgroups every SIMD is refilled on its own (+0.9 % over 4-wave workgroups, A/B)
#endif
#ifndef NERF_F32_HACK_NOBIAS
#define NERF_F32_HACK_NOBIAS 0
#endif
#ifndef NERF_F32_HACK_NOSAVE        // timing-only: the SAVE instance computes everything but stores no activation
#define NERF_F32_HACK_NOSAVE 0
#endif
#ifndef NERF_BWD_HACK_NOMASK        // timing-only: the backward chain skips the ReLU masks (no activation reads)
#define NERF_BWD_HACK_NOMASK 0
#endif

// The tail of the packed stream (9 layer biases, views bias, sigma / rgb head weights: 12 KiB) is staged in LDS by twelve
// asynchronous LDS-DMAs issued before the positional encoding is computed, so the 32 bias reads at every layer boundary
// and the head-weight reads are ds_read_b128 with ~100 cycles of latency instead of global loads with > 1000 -- with one
// wave per SIMD that latency was exposed ten times per tile (round 1 measured the boundary bias loads at 1.7 %).
constexpr int kTailFloats = 3072;                      // [kOffBias, kOffBias + 3072): everything but the 4 head biases
static_assert(nerf::kOffHeadBias - nerf::kOffBias == kTailFloats, "LDS tail = biases + views bias + head weights");
template <int NT>
__device__ __forceinline__ void load_bias(f32x16 (&acc)[NT], lds_cfloat* bias_h) {
  lds_cf32x4* b = reinterpret_cast<lds_cf32x4*>(bias_h);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v = NERF_F32_HACK_NOBIAS ? f32x4{0.f, 0.f, 0.f, 0.f} : b[j * 4 + q];
      acc[j][4 * q + 0] = v.x; acc[j][4 * q + 1] = v.y; acc[j][4 * q + 2] = v.z; acc[j][4 * q + 3] = v.w;
    }
  }
}

// The weight stream: one 1-KiB block (64 lanes x float4) per step, consumed strictly in memory
// order through the whole network, so a register ring prefetched kPF blocks ahead runs across
// layer boundaries without ever draining (every layer has a multiple of kRing steps).
constexpr int kRing = 16;   // ring slots (4 VGPRs each)
constexpr int kPF = 8;       // blocks in flight ahead of the consumer

// A "tap" is called once per 4-k-step group of a GEMM with the (tile, quad) of the INPUT registers that group consumes,
// X[t][4q .. 4q+3] = features 32t + 8q + 4h + (0..3) of the lane's point.  The training kernels use it to store an
// activation (or gradient) row WHILE the next layer consumes it -- one 16-byte store per 32 MFMAs, spread over the
// layer -- instead of 32 stores back to back after the producing layer: every s_waitcnt vmcnt(N) of the weight ring
// also waits for older stores (one in-order counter), so a burst of stores exposed their full write latency once per
// layer (measured: 1.64 ms of an 8.2 ms SAVE forward, 1.0 ms of the backward chain, tools/ab_train.py).
#ifndef NERF_SAVE_TAPS
#define NERF_SAVE_TAPS 1
#endif
struct NoTap { static constexpr bool kIsTap = false; __device__ __forceinline__ void operator()(int, int, const f32x16&) const {} };
// store the quad to its row-major [point][feature] row
struct SignBits { unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u; };     // bit 16*(t&1) + 4q + e of word t>>1 (scalars: stays in registers)
template <bool GRAD, bool BITS = false>   // GRAD: a gradient row of the backward chain (only the timing switches differ)
struct StoreTap {
  static constexpr bool kIsTap = true;
  float* row;              // this lane's row + 4h
  SignBits* sb;            // BITS: collects the sign bits of the row on the way (compile-time switch: no branch, no array)
  __device__ __forceinline__ void operator()(int t, int q, const f32x16& Xt) const {
    f32x4 v;
    v.x = Xt[4 * q + 0]; v.y = Xt[4 * q + 1]; v.z = Xt[4 * q + 2]; v.w = Xt[4 * q + 3];
    // the store wants its four values in CONSECUTIVE registers; without this opaque redefinition the allocator tries to
    // keep all 32 quads of the (element-wise live) activation set in aligned consecutive registers for the whole layer and
    // ends up shuffling 130 registers through scratch at the layer boundaries -- four moves per group are cheaper
    asm volatile("" : "+v"(v));
    if (!(GRAD ? 0 : NERF_F32_HACK_NOSAVE)) {
      *reinterpret_cast<f32x4*>(row + 32 * t + 8 * q) = v;
    }
    if constexpr (BITS) {
      // the rows that carry sign bits are post-ReLU (integer max: >= +0, never -0), so "positive" == "bit pattern != 0":
      // v_min_u32 + v_lshl_or per value instead of compare + select + or
      auto nz = [](float x) { const unsigned u = __float_as_uint(x); return u < 1u ? u : 1u; };
      const unsigned m = (nz(v.x) | (nz(v.y) << 1) | (nz(v.z) << 2) | (nz(v.w) << 3)) << (16 * (t & 1) + 4 * q);
      switch (t >> 1) {                  // (t is a constant once the GEMM loop is unrolled)
        case 0: sb->w0 |= m; break;
        case 1: sb->w1 |= m; break;
        case 2: sb->w2 |= m; break;
        default: sb->w3 |= m; break;
      }
    }
  }
};
template <bool ON, bool BITS>
__device__ __forceinline__ auto save_tap(float* row, SignBits* sb) {
  if constexpr (ON && NERF_SAVE_TAPS) return StoreTap<false, BITS>{row, sb};
  else return NoTap{};
}

// The stream is consumed through inline-asm loads (every instance, training and backward included).  What that buys
// over loads the compiler schedules: (1) the loads use the scalar-base form
// `global_load_dwordx4 v, v_laneoff, s[base] offset:imm` (no per-load 64-bit VALU address); (2) ONE
// `s_waitcnt vmcnt(kPF)` per k-group instead of the eight the compiler places in front of the first row's MFMAs --
// with one wave per SIMD every instruction issued between MFMAs is time off the matrix pipe.
struct AStream {
  const char* base;        // (uniform) byte address of block 0 of the NEXT block to consume
  unsigned voff;           // this lane's byte offset inside a block (lane * 16)
  f32x4 ring[kRing];
};
// (an "a"-constrained ring, i.e. loads straight into AGPRs, gave wrong results: the ring is "v"-constrained)
// blocks [first, first + N) relative to as.base into ring slots (slot0 + k) % kRing; the immediate offset field is
// 13-bit signed, so every four blocks get their own scalar base
template <int N, int K = 0>
__device__ __forceinline__ void astream_load(AStream& as, int first, int slot0) {
  if constexpr (K < N) {
    const char* b = as.base + (long long)(first + (K & ~3)) * 1024;
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3"
                 : "=&v"(as.ring[(slot0 + K) % kRing]) : "v"(as.voff), "s"(b), "n"((K & 3) * 1024) : "memory");
    astream_load<N, K + 1>(as, first, slot0);
  }
}
// one block (first + K) into ring slot (slot0 + K) % kRing, same addressing as astream_load
template <int K>
__device__ __forceinline__ void astream_load_one(AStream& as, int first, int slot0) {
  const char* b = as.base + (long long)(first + (K & ~3)) * 1024;
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3"
               : "=&v"(as.ring[(slot0 + K) % kRing]) : "v"(as.voff), "s"(b), "n"((K & 3) * 1024) : "memory");
}
// Group P > 0 of a GEMM is the first to run after a prefix of dead groups (gemm_tiles): its eight blocks into its own ring
// half, slots 0..7 for even P and 8..15 for odd P, as the static slots of the group's code expect.  P = 0: nothing (group 0
// was prefetched by the previous GEMM).  ONE asm statement with its branches inside, once per GEMM, so the compiler sees
// straight-line code in which every slot passes through a read-write operand: with the loads in a conditional block of their
// own it copied the slots where the paths join, while the loads were in flight.  Everything older is waited for first -- the
// prefetch for group 0, issued before the decision was possible, may still be in flight into the same slots (it was issued
// a group earlier: normally free).  P comes back opaque: the groups' `g < P` tests stay one scalar compare each.
__device__ __forceinline__ void astream_fetch_from(AStream& as, unsigned& P) {
  const char* b0 = as.base + (long long)P * (8 * 1024);
  const char* b1 = b0 + 4096;
  asm volatile("s_cmp_eq_u32 %[P], 0\n\t"
               "s_cbranch_scc1 .Lpre_done_%=\n\t"
               "s_waitcnt vmcnt(0)\n\t"
               "s_bitcmp1_b32 %[P], 0\n\t"
               "s_cbranch_scc1 .Lpre_odd_%=\n\t"
               "global_load_dwordx4 %0, %[vo], %[b0]\n\t"
               "global_load_dwordx4 %1, %[vo], %[b0] offset:1024\n\t"
               "global_load_dwordx4 %2, %[vo], %[b0] offset:2048\n\t"
               "global_load_dwordx4 %3, %[vo], %[b0] offset:3072\n\t"
               "global_load_dwordx4 %4, %[vo], %[b1]\n\t"
               "global_load_dwordx4 %5, %[vo], %[b1] offset:1024\n\t"
               "global_load_dwordx4 %6, %[vo], %[b1] offset:2048\n\t"
               "global_load_dwordx4 %7, %[vo], %[b1] offset:3072\n\t"
               "s_branch .Lpre_done_%=\n"
               ".Lpre_odd_%=:\n\t"
               "global_load_dwordx4 %8, %[vo], %[b0]\n\t"
               "global_load_dwordx4 %9, %[vo], %[b0] offset:1024\n\t"
               "global_load_dwordx4 %10, %[vo], %[b0] offset:2048\n\t"
               "global_load_dwordx4 %11, %[vo], %[b0] offset:3072\n\t"
               "global_load_dwordx4 %12, %[vo], %[b1]\n\t"
               "global_load_dwordx4 %13, %[vo], %[b1] offset:1024\n\t"
               "global_load_dwordx4 %14, %[vo], %[b1] offset:2048\n\t"
               "global_load_dwordx4 %15, %[vo], %[b1] offset:3072\n"
               ".Lpre_done_%=:"
               : "+v"(as.ring[0]), "+v"(as.ring[1]), "+v"(as.ring[2]), "+v"(as.ring[3]), "+v"(as.ring[4]), "+v"(as.ring[5]),
                 "+v"(as.ring[6]), "+v"(as.ring[7]), "+v"(as.ring[8]), "+v"(as.ring[9]), "+v"(as.ring[10]), "+v"(as.ring[11]),
                 "+v"(as.ring[12]), "+v"(as.ring[13]), "+v"(as.ring[14]), "+v"(as.ring[15]), [P] "+s"(P)
               : [vo] "v"(as.voff), [b0] "s"(b0), [b1] "s"(b1) : "memory", "scc");
}
// the N ring slots from slot0 on are about to be read: one wait for everything but the CNT newest vector-memory
// operations (normally the kPF blocks issued for the next group; fewer at the end of a tile's stream)
template <int N, int CNT = 8>
__device__ __forceinline__ void astream_wait(AStream& as, int slot0) {
  static_assert(N == 2 || N == 4 || N == 8, "blocks per k-group");
  static_assert(CNT >= 0 && CNT <= 9, "outstanding operations allowed");
  if constexpr (N == 8)
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(as.ring[(slot0 + 0) % kRing]), "+v"(as.ring[(slot0 + 1) % kRing]), "+v"(as.ring[(slot0 + 2) % kRing]),
                   "+v"(as.ring[(slot0 + 3) % kRing]), "+v"(as.ring[(slot0 + 4) % kRing]), "+v"(as.ring[(slot0 + 5) % kRing]),
                   "+v"(as.ring[(slot0 + 6) % kRing]), "+v"(as.ring[(slot0 + 7) % kRing]) : "n"(CNT) : "memory");
  else if constexpr (N == 4)
    asm volatile("s_waitcnt vmcnt(%4)"
                 : "+v"(as.ring[(slot0 + 0) % kRing]), "+v"(as.ring[(slot0 + 1) % kRing]), "+v"(as.ring[(slot0 + 2) % kRing]),
                   "+v"(as.ring[(slot0 + 3) % kRing]) : "n"(CNT) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(as.ring[(slot0 + 0) % kRing]), "+v"(as.ring[(slot0 + 1) % kRing]) : "n"(CNT) : "memory");
}
// Before code that is not a k-group loop (heads, late encodings) every outstanding asm load is waited for, so that
// whatever the compiler then does with ring registers (copy, spill, reuse around the foreign code) moves landed data.
__device__ __forceinline__ void stream_drain(AStream& as) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(as.ring[0]), "+v"(as.ring[1]), "+v"(as.ring[2]), "+v"(as.ring[3]), "+v"(as.ring[4]), "+v"(as.ring[5]),
                 "+v"(as.ring[6]), "+v"(as.ring[7]), "+v"(as.ring[8]), "+v"(as.ring[9]), "+v"(as.ring[10]), "+v"(as.ring[11]),
                 "+v"(as.ring[12]), "+v"(as.ring[13]), "+v"(as.ring[14]), "+v"(as.ring[15]) :: "memory");
}
// after a wave-uniform early exit the compiler's divergence analysis no longer proves the stream base uniform (it would
// feed a VGPR pair to the "s" operand of the asm loads): re-assert it, two v_readfirstlane
__device__ __forceinline__ void stream_reassert_uniform(AStream& as) {
  const unsigned long long b = reinterpret_cast<unsigned long long>(as.base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  as.base = reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void wstream_start(AStream& as, const f32x4* p_lane0, int lane) {
  as.base = reinterpret_cast<const char*>(p_lane0);
  as.voff = (unsigned)lane * 16u;
  astream_load<8>(as, 0, 0);
}
// acc[j] += W(j, :) . X   over KT input tiles (16 k-steps each).
// Interleaved form: the NT blocks of a 4-k-step group are consumed component by component, so
// consecutive MFMAs always hit different accumulators (no back-to-back dependent MFMAs); the ring
// (2 x 8 blocks) holds the current group(s) while the next 8 blocks of the stream are in flight.
// LAST: the stream of this tile ends with this call.  The asm loads must not prefetch past the end: the compiler sees
// those ring registers as dead and reuses them while the loads are still in flight (found by scanning the ISA: the
// rgb-head temporaries landed in v[0:3] of the ring).  So the last groups issue no loads and wait for
// correspondingly fewer outstanding ones.
//
// KSKIP (inference instances, GEMMs whose B operand is a ReLU output): a k-step whose activation register is +0 in all 64
// lanes -- both of its features are off at every point of the tile -- would add fma(a, +0, C) = C to every accumulator
// (finite a), so its NT MFMAs sit behind one wave-uniform branch.  The decision is one v_cmp on the BIT PATTERN (a NaN keeps
// its row alive; so do the padding lanes of a ragged tile) against `kthr` and a branch on the lane mask, in the shadow of the
// MFMAs issued before it: kthr = 1 asks "any lane non-zero", kthr = 0 (MlpArgs::skip_dead_ksteps off) is true for every
// row.  A skipped row leaves an accumulator that is -0 as -0 where the MFMA would have made it +0: the integer-max ReLU
// that every such tile goes through next maps both to +0.  The next group's loads are issued whether or not row 0 runs:
// behind its first four MFMAs as before, back to back (between not-taken branches) when it is dead; ring slots and wait
// counts do not change.
// -> the mask of lanes that keep the k-step of register x alive (a scalar pair; 0 = skip)
__device__ __forceinline__ unsigned long long kstep_live(float x, unsigned kthr) {
  return __builtin_amdgcn_ballot_w64(__float_as_uint(x) >= kthr);
}
#ifndef NERF_F32_ASM_OVERRUN
#define NERF_F32_ASM_OVERRUN 0      // 1 re-creates the prefetch past the stream end (a known hazard: self-test of tools/check_asm_stream.py)
#endif
// -> group g of a GEMM is dead: none of its four k-steps is alive in any lane
__device__ __forceinline__ bool group_dead(const unsigned long long (&live4)[4]) {
  return ((live4[0] | live4[1]) | (live4[2] | live4[3])) == 0ull;
}
template <int KT, int NT, bool LAST = false, class TAP = NoTap, bool KSKIP = false>
__device__ __forceinline__ void gemm_tiles(f32x16 (&acc)[NT], const f32x16 (&X)[KT], AStream& as, TAP tap = TAP(), unsigned kthr = 0u,
                                           bool prefix = false) {
  static_assert(kRing == 16 && kPF == 8, "interleaved form: ring 16, 8 blocks in flight");
  static_assert(!KSKIP || !TAP::kIsTap, "k-step skipping: inference instances only");
  static_assert((KT * 4 * NT) % kRing == 0, "layer steps must be a multiple of the ring");
  static_assert(!LAST || (kPF % NT == 0 && KT * 4 * NT >= 2 * kPF), "tail handling: whole groups");
  constexpr int kBlocks = KT * 4 * NT;
  // Leading dead groups (KSKIP, spread form).  P, the length of the run of all-dead groups this GEMM's input starts with, is
  // counted here, before the first group: four decisions per group until the first that has a live row.  Groups g < P are
  // stepped over with nothing issued -- no wait, no loads, no row branches, one scalar compare -- and group P first finds its
  // own eight blocks fetched into its own (static) slots (astream_fetch_from); from there the code is the one it always was.
  // The last group is never counted in (P <= 31): it always runs and issues the next GEMM's prefetch, so the stream never stalls
  // across a layer boundary, and in a LAST call it is the stream end: nothing is fetched past it.  `prefix` is only ever set
  // with kthr != 0 (MlpArgs::skip_dead_groups).
  constexpr bool kPrefix = KSKIP && NT == 8 && !(LAST && NERF_F32_ASM_OVERRUN);
  unsigned P = 0u;
  if constexpr (kPrefix) {
    // The fetch's slots are read-write operands, which would keep the whole ring alive across the layer boundary in front of
    // this call (+32 registers there: the full instances spilled).  Only slots 0..7 hold anything then, the prefetch for group
    // 0; the upper half was consumed by the last group of the previous GEMM and nothing is in flight into it: cut it off.
    // That rests on the assert above, not on the order of the calls: every call consumes a multiple of kRing blocks, so every
    // call starts at slot 0, and a call with NT = 8 (all that precede a call with a prefix in the packed stream) therefore
    // has an even number of groups and ends in slots 8..15; its last group prefetches this call's group 0 into slots 0..7.
#pragma unroll
    for (int k = kRing / 2; k < kRing; ++k) asm volatile("" : "=v"(as.ring[k]));
    if (prefix) {
#pragma unroll
      for (int g = 0; g + 1 < KT * 4; ++g) {
        unsigned long long live4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) live4[q] = kstep_live(X[g >> 2][(g & 3) * 4 + q], kthr);
        if (!group_dead(live4)) break;
        P = g + 1;
      }
    }
    astream_fetch_from(as, P);
  }
  if constexpr (KSKIP) {
    // the accumulators (just initialised from the LDS bias reads) are made ready HERE, once: with every row behind a branch
    // the compiler cannot tell which row first touches an accumulator, and repeats the `s_waitcnt lgkmcnt` ladder of those
    // reads in front of the MFMAs of all 128 rows of the layer (measured: 8 % less code, the same time)
    if constexpr (NT == 8)
      asm volatile("" : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]), "+a"(acc[4 % NT]), "+a"(acc[5 % NT]), "+a"(acc[6 % NT]), "+a"(acc[7 % NT]));
    else
      asm volatile("" : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3]));
  }
#pragma unroll
  for (int g = 0; g < KT * 4; ++g) {
    if constexpr (NT == 8 && !TAP::kIsTap && !(LAST && NERF_F32_ASM_OVERRUN)) {      // (GEMMs with a storing tap: the spread form measured 2.8 % SLOWER)
      // Spread form (the 8-out-tile GEMMs = 90 % of the MFMAs): the eight loads of the NEXT group are not issued back to
      // back at the group start -- 8 x ~16 cycles of vector-memory issue during which this wave, alone on its SIMD,
      // feeds the matrix pipe nothing -- but two behind each of the first four MFMAs, where a 64-cycle MFMA covers them.
      // The group's own blocks were the last loads issued (during the previous group): the wait is vmcnt(0) -- also in the
      // LAST GEMM of a stream, whose final group simply issues nothing (layer 7 of the inference instances).
      const bool kMore = !LAST || g * NT + kPF < kBlocks;      // (g is a constant once the loop is unrolled)
      const int t = g >> 2, r0 = (g & 3) * 4;
      if constexpr (KSKIP) {
        if (g + 1 < KT * 4 && (unsigned)g < P) continue;      // leading dead group (P = 0 with the path off)
      }
      astream_wait<NT, 0>(as, (g * NT) % kRing);
      __builtin_amdgcn_sched_barrier(0);
      tap(t, g & 3, X[t]);
      // KSKIP: the four decisions of the group are taken here, behind the previous group's last MFMA, into four scalar pairs;
      // a row then costs one s_cmp and one branch.  Decided row by row (v_cmp -> vcc -> s_cbranch_vccz in front of each row)
      // the same kernel measured 50 ms slower per 1150 ms frame, with the skipping on as well as off.
      unsigned long long live4[4] = {0ull, 0ull, 0ull, 0ull};
      if constexpr (KSKIP) {
#pragma unroll
        for (int q = 0; q < 4; ++q) live4[q] = kstep_live(X[t][r0 + q], kthr);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (KSKIP) {
          unsigned long long live = live4[q];
          if (q == 0 && kMore) {
            // row 0 carries the next group's loads.  They stay ONE copy each, in straight-line code between five branches
            // on the same decision (with the loads duplicated into a dead-row arm the compiler stopped accumulating in
            // place and copied 128 accumulator registers at the join); the decision is made opaque before each branch so
            // that the branches are not threaded back into two arms.
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              asm volatile("" : "+s"(live));
              if (live) acc[j] = mfma32(as.ring[(g * NT + j) % kRing][0], X[t][r0], acc[j]);
              __builtin_amdgcn_sched_barrier(0);
              if (j == 0) { astream_load_one<0>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<1>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
              if (j == 1) { astream_load_one<2>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<3>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
              if (j == 2) { astream_load_one<4>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<5>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
              if (j == 3) { astream_load_one<6>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<7>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
              __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("" : "+s"(live));
            if (live) {
#pragma unroll
              for (int j = 4; j < NT; ++j) acc[j] = mfma32(as.ring[(g * NT + j) % kRing][0], X[t][r0], acc[j]);
            }
          } else if (live) {
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = mfma32(as.ring[(g * NT + j) % kRing][q], X[t][r0 + q], acc[j]);
          }
          continue;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const f32x4 a = as.ring[(g * NT + j) % kRing];
          acc[j] = mfma32(a[q], X[t][r0 + q], acc[j]);
          if (q == 0 && j < 4 && kMore) {
            __builtin_amdgcn_sched_barrier(0);
            if (j == 0) { astream_load_one<0>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<1>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
            if (j == 1) { astream_load_one<2>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<3>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
            if (j == 2) { astream_load_one<4>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<5>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
            if (j == 3) { astream_load_one<6>(as, g * NT + kPF, (g * NT + kPF) % kRing); astream_load_one<7>(as, g * NT + kPF, (g * NT + kPF) % kRing); }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      continue;
    } else if constexpr (!LAST || NERF_F32_ASM_OVERRUN) {
      astream_load<NT>(as, g * NT + kPF, (g * NT + kPF) % kRing);
      // everything but the kPF newest loads has landed: this group's blocks.  A storing tap's row store of the previous
      // group is older than those loads, so vmcnt(kPF) waits for it too; vmcnt(kPF + 1), which leaves it in flight,
      // measured 5 % SLOWER on the SAVE forward (store latency is not what the taps cost).  Both calls wait for vmcnt(kPF);
      // they stay two call sites because merging them changes the schedule the compiler emits for the SAVE instances
      if (g == 0) astream_wait<NT>(as, (g * NT) % kRing);            // (first group of a call: no tap store issued yet)
      else astream_wait<NT, kPF>(as, (g * NT) % kRing);
    } else {
      // tail of the tile's stream: nothing is issued past its end, and the wait allows only the loads that really are
      // younger than this group's blocks (g is a constant once the loop is unrolled: the switch folds to one case)
      if (g * NT + kPF < kBlocks) astream_load<NT>(as, g * NT + kPF, (g * NT + kPF) % kRing);
      const int younger = kBlocks - (g + 1) * NT < kPF ? kBlocks - (g + 1) * NT : kPF;
      switch (younger) {
        case 8: astream_wait<NT, 8>(as, (g * NT) % kRing); break;
        case 6: astream_wait<NT, 6>(as, (g * NT) % kRing); break;
        case 4: astream_wait<NT, 4>(as, (g * NT) % kRing); break;
        case 2: astream_wait<NT, 2>(as, (g * NT) % kRing); break;
        default: astream_wait<NT, 0>(as, (g * NT) % kRing); break;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    const int t = g >> 2, r0 = (g & 3) * 4;
    tap(t, g & 3, X[t]);               // (after the wait: a store here is older than the next group's loads, see vmcnt note above)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (KSKIP) {
        if (!kstep_live(X[t][r0 + q], kthr)) continue;      // (this form issued the next group's loads above)
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const f32x4 a = as.ring[(g * NT + j) % kRing];
        acc[j] = mfma32(a[q], X[t][r0 + q], acc[j]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  as.base += (long long)KT * 4 * NT * 1024;
}

// ReLU as a signed-integer max on the bit pattern (negative floats and -0 are negative integers): one VALU
// instruction per value; fmaxf costs two (the compiler first canonicalises a possible signalling NaN), and with one
// wave per SIMD these 128 values per layer are issued with the matrix pipe drained.  NaNs pass through unchanged.
// SAVE: ReLU that also returns the sign bits of the layer (bit 16*(t&1) + r of word t>>1 <-> register r of tile t is
// positive) for the backward chain's masks.  The bits are collected HERE, where every value passes through a VGPR anyway
// (two more VALU per value on the drained pipe, +1.5 % of the forward); collecting them inside the consuming GEMM's
// tap would hide that time but made the kernel spill 130 registers.
template <int NT>
__device__ __forceinline__ u32x4 relu_bits_tiles(f32x16 (&acc)[NT]) {
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int v = __float_as_int(acc[j][r]);
      const int rl = v > 0 ? v : 0;                                  // integer ReLU (see relu_tiles)
      acc[j][r] = __int_as_float(rl);
      w[j >> 1] |= ((unsigned)rl < 1u ? 0u : 1u) << (16 * (j & 1) + r);
    }
  u32x4 b; b.x = w[0]; b.y = w[1]; b.z = w[2]; b.w = w[3];
  return b;
}
template <int NT>
__device__ __forceinline__ void relu_tiles(f32x16 (&acc)[NT]) {
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int bits = __float_as_int(acc[j][r]);        // ReLU as a signed-integer max on the bit pattern: one VALU per value
      acc[j][r] = __int_as_float(bits > 0 ? bits : 0);   // (fmaxf costs two: sNaN canonicalisation)
    }
}

// DENS: stop after the sigma head (MlpArgs::density_only).  DSKIP (MlpArgs::skip_dead_colour): a tile whose 32 points all have
// sigma <= 0 stops after the sigma head too -- relu(sigma) = 0 gives alpha = 0 and weight 0, so compositing multiplies those
// colours by exactly zero -- and writes (0, 0, 0, sigma); every other tile runs in full, bit for bit as the plain instance.
// SAVE && DSKIP (training forward of the fine pass): such a tile also stores nothing past h6 -- compositing's adjoint hands it
// a zero gradient, so the backward pass (which works on live tiles only) never reads its h7 / feature / views rows.
template <bool RAY_MODE, bool SAVE = false, bool DENS = false, bool DSKIP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_mlp_f32_kernel(MlpArgs a) {
  static_assert(!(DSKIP && DENS), "dead-colour skipping is a variant of the full network");
  using namespace nerf;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int h = lane >> 5;
  const long long n_points = a.index ? (long long)*a.count : a.n_points;   // masked pass: device-side count
  const long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  const long long base = tile * kTilePts;
  // Tile shape (MlpArgs::tile_rays_log2, inference ray instances, no list): tile T holds R = 1 << lg neighbouring rays by
  // sps = 32 >> lg consecutive samples; q = n_samples / sps tiles cover one group of R rays.  Everything below the prologue
  // sees (p, ray, s, valid) per lane and nothing else, so the shape changes which k-steps are dead, never a value.
  const int lg = (RAY_MODE && !SAVE) ? a.tile_rays_log2 : 0;
  const long long pl = base + (lane & 31);
  long long p, ray;                                    // global point id (output slot), its ray
  int s;
  bool valid;
  if (lg != 0) {
    const long long n_rays = n_points / a.n_samples;
    const int q = a.n_samples >> (5 - lg);
    const long long g = tile / q;                      // ray group
    if ((g << lg) >= n_rays) return;                   // whole wave idle: T >= ceil(n_rays / R) * q
    const int j = lane & 31;
    const long long r = (g << lg) + (j >> (5 - lg));
    valid = r < n_rays;
    ray = valid ? r : n_rays - 1;                      // ragged group: repeat the last ray's point, store nothing
    s = ((int)(tile - g * q) << (5 - lg)) + (j & ((32 >> lg) - 1));
    p = ray * a.n_samples + s;
  } else {
    if (base >= n_points) return;                      // whole wave idle (no barriers in this kernel)
    valid = pl < n_points;
    const long long plc = valid ? pl : n_points - 1;
    p = a.index ? (long long)a.index[plc] : plc;
    ray = p / a.n_samples;
    s = (int)(p - ray * a.n_samples);
  }
  {
  const long long pc = p;

  // 12 KiB per wave of the workgroup, + 1 KiB behind it for the folded views bias (instances with a colour branch)
  constexpr int kTailLds = kTailFloats + (DENS ? 0 : 256);
  __shared__ __attribute__((aligned(16))) float tail_smem[NERF_F32_WG_WAVES * kTailLds];
  lds_char* const tail_w = (lds_char*)tail_smem + wave * (kTailLds * 4);
  {
    const char* src = reinterpret_cast<const char*>(a.packed + kOffBias) + lane * 16;
#pragma unroll
    for (int i = 0; i < kTailFloats * 4 / 1024; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void*)(src + i * 1024),
                                       (lds_void*)(tail_w + i * 1024), 16, 0, 0);
    if constexpr (!DENS)
      __builtin_amdgcn_global_load_lds((gbl_void*)(reinterpret_cast<const char*>(a.fold + kFoldOffBias) + lane * 16),
                                       (lds_void*)(tail_w + kTailFloats * 4), 16, 0, 0);
  }
  lds_cfloat* const tail = reinterpret_cast<lds_cfloat*>(tail_w);

  // ---- point + view direction -----------------------------------------------------------
  float x[3], d[3];
  if (RAY_MODE) {
    const float t = a.tvals[ray * a.t_ray_stride + s];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float dc = a.rays_d[ray * 3 + c];
      x[c] = __fadd_rn(a.rays_o[ray * 3 + c], __fmul_rn(dc, t));   // o + d*t, two roundings
      d[c] = dc;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = a.pts[pc * 3 + c];
  }
  if (a.viewdirs != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = a.viewdirs[ray * 3 + c];
  } else {
    const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2]));
    const float nrm = __fsqrt_rn(n2);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = __fdiv_rn(d[c], nrm);
  }

  // ---- positional encoding straight into B-operand layout (nerf_layout.h pe_*_feat) -------
  // ocml's sincosf stays: the Cody-Waite sincos of the f32x / backward kernels (1e-7 abs) measured +0.57 % here, but raw
  // moves by up to 1.1e-4 and a different ray of the white-noise parity scene flips (PSNR 65 -> 49 dB on that fixture)
  f32x16 PE[2], DPE[1];
  {
    const float hs = h ? 32.0f : 1.0f;                 // lane-half 1 evaluates octaves 5..9
#pragma unroll
    for (int ai = 0; ai < 15; ++ai) {
      const float arg = x[ai % 3] * (hs * (float)(1 << (ai / 3)));   // exact: power-of-two scale
      float sv, cv;
      sincosf(arg, &sv, &cv);      // ocml: <= 2 ulp of the reference's sin / cos at arguments up to 3000 rad
      PE[(2 * ai) >> 4][(2 * ai) & 15] = sv;
      PE[(2 * ai + 1) >> 4][(2 * ai + 1) & 15] = cv;
    }
    PE[1][14] = h ? x[2] : x[0];
    PE[1][15] = h ? 0.0f : x[1];
  }
  // direction encoding: the training forward needs it now (it is stored with the other encodings); the inference
  // instances compute it right before the views layer from the three direction components -- kept live through the
  // trunk, its 16 registers were spilled to scratch and back (8.5 GB of scratch writes per frame in the counters)
  auto encode_dir = [&]() {
    const float ds = h ? 4.0f : 1.0f;                  // lane-half 1 evaluates octaves 2,3
#pragma unroll
    for (int ai = 0; ai < 6; ++ai) {
      const float arg = d[ai % 3] * (ds * (float)(1 << (ai / 3)));
      float sv, cv;
      sincosf(arg, &sv, &cv);      // ocml: <= 2 ulp of the reference's sin / cos at arguments up to 3000 rad
      DPE[0][2 * ai] = sv;
      DPE[0][2 * ai + 1] = cv;
    }
    DPE[0][12] = h ? d[2] : d[0];
    DPE[0][13] = h ? 0.0f : d[1];
    DPE[0][14] = 0.0f;
    DPE[0][15] = 0.0f;
  };
  // SAVE: rows are stored unconditionally -- the idle lanes of a ragged last tile write the padding rows every
  // TrainSave region has (pad32), so none of the ~300 stores of a tile needs an exec mask
  const long long ps = pl;
  if (SAVE) encode_dir();
  if (SAVE && !NERF_F32_HACK_NOSAVE) {          // encodings in reference channel order (slot -> channel: nerf_layout.h)
    float* pe_row = a.save + TrainSave::off_pe(a.n_points) + ps * 64;
#pragma unroll
    for (int n = 0; n < 32; ++n) {
      const int c0 = pe_xyz_feat(n, 0), c1 = pe_xyz_feat(n, 1);
      const int c = h ? c1 : c0;
      if (c >= 0) pe_row[c] = PE[n >> 4][n & 15];
    }
    if (h) pe_row[63] = 0.0f;
    float* dpe_row = a.save + TrainSave::off_dpe(a.n_points) + ps * 32;
#pragma unroll
    for (int n = 0; n < 16; ++n) {
      const int c0 = pe_dir_feat(n, 0), c1 = pe_dir_feat(n, 1);
      const int c = h ? c1 : c0;
      if (c >= 0) dpe_row[c] = DPE[0][n];
    }
    if (h) { dpe_row[27] = 0.f; dpe_row[28] = 0.f; dpe_row[29] = 0.f; dpe_row[30] = 0.f; dpe_row[31] = 0.f; }
  }

  const float* __restrict__ pk = a.packed;
  // running weight stream.  The asm loads are asynchronous behind the compiler's back: were it to spill or copy a ring
  // register between a load and the group's s_waitcnt it would move stale data (wrong results, or a fault).  So every
  // instance is proven hazard-free on its ISA by tools/check_asm_stream.py (every build, and the CPU test suite).
  AStream ws;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // the tail DMAs (issued before the encodings) have landed
  wstream_start(ws, reinterpret_cast<const f32x4*>(pk), lane);
  lds_cfloat* bias = tail + h * 128;                                 // + 256 per layer

  // SAVE: every activation row is stored by the GEMM that CONSUMES it (tap, one 16-byte store per 4-k-step group); the
  // ReLU sign bits of a layer are collected by its ReLU pass and stored at once (one coalesced 16-byte store per lane)
  float* const srow = SAVE ? a.save + ps * 256 + 4 * h : nullptr;                      // + region offset
  u32x4* const bits_out = SAVE ? reinterpret_cast<u32x4*>(a.save + TrainSave::off_bits(a.n_points) +
                                                          TrainSave::bits_block(base / kTilePts, 0)) + lane : nullptr;
  SignBits sb;                                                  // collected by the consuming GEMM's tap
  constexpr bool kTapBits = SAVE;
  auto tap_bits_done = [&](int which) {
    if constexpr (kTapBits) {
      u32x4 b; b.x = sb.w0; b.y = sb.w1; b.z = sb.w2; b.w = sb.w3;
      if (!NERF_F32_HACK_NOSAVE) bits_out[which * 64] = b;
      sb = SignBits();
    }
  };
  auto relu8 = [&](f32x16 (&A)[8], int which) {
    relu_tiles<8>(A);
  };

  // inference instances: k-steps whose activation register is zero tile-wide are skipped (gemm_tiles KSKIP) in every GEMM
  // fed by a ReLU output -- not in the PE / direction GEMMs, whose inputs are not ReLU outputs, and not in the training forward
  constexpr bool kKSkip = !SAVE;
  const unsigned kthr = a.skip_dead_ksteps ? 1u : 0u;                // (wave-uniform kernel argument)
  const bool kpre = a.skip_dead_ksteps && a.skip_dead_groups;       // leading dead groups of each such GEMM are stepped over
  using TrunkTap = decltype(save_tap<SAVE, kTapBits>(srow, &sb));

  f32x16 X[8], Y[8];
  // L0: PE(64) -> 256
  load_bias<8>(X, bias);
  gemm_tiles<2, 8>(X, PE, ws);
  relu8(X, 0);

  float sigma = 0.0f;
  constexpr int kPairs = 3;                           // layer 7 is peeled off below: every instance ends or restarts its stream there
  // not unrolled: unrolled by two the compiler saves the register shuffles at the back edge, but twice the code measured
  // 2.5 % SLOWER (instruction cache)
#pragma unroll 1
  for (int pr = 0; pr < kPairs; ++pr) {
    // X -> Y : L1, L3, L5   (consumes h0, h2, h4)
    load_bias<8>(Y, bias + (1 + 2 * pr) * 256);
    if (pr == 2) {                                     // skip connection: cat([pts63, h]) (network.py:58)
      gemm_tiles<2, 8>(Y, PE, ws);
    }
    gemm_tiles<8, 8, false, TrunkTap, kKSkip>(Y, X, ws, save_tap<SAVE, kTapBits>(srow + TrainSave::off_h(a.n_points, 2 * pr), &sb), kthr, kpre);
    tap_bits_done(2 * pr);
    relu8(Y, 1 + 2 * pr);
    // Y -> X : L2, L4, L6   (consumes h1, h3, h5)
    load_bias<8>(X, bias + (2 + 2 * pr) * 256);
    gemm_tiles<8, 8, false, TrunkTap, kKSkip>(X, Y, ws, save_tap<SAVE, kTapBits>(srow + TrainSave::off_h(a.n_points, 1 + 2 * pr), &sb), kthr, kpre);
    tap_bits_done(1 + 2 * pr);
    relu8(X, 2 + 2 * pr);
  }

  if constexpr (DENS) {
    // density only (the coarse pass of a hierarchical render or training step: the reference uses nothing but its sigma,
    // volume_renderer.py:335): layer 7, the sigma head, and out.  This GEMM is the LAST of the tile: the asm ring must not
    // prefetch past it (the compiler reuses ring registers it sees as dead).  Nothing downstream of h7 exists here, so
    // (SAVE) its row and sign bits are stored directly.  The sigma arithmetic is the full instance's, bit for bit.
    load_bias<8>(Y, bias + 7 * 256);
    gemm_tiles<8, 8, true, TrunkTap, kKSkip>(Y, X, ws, save_tap<SAVE, kTapBits>(srow + TrainSave::off_h(a.n_points, 6), &sb), kthr, kpre);
    tap_bits_done(6);
    relu8(Y, 7);
    lds_cf32x4* wa = reinterpret_cast<lds_cf32x4*>(tail + (kOffWAlpha - kOffBias) + h * 128);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w4 = wa[t * 4 + q];
        acc0 = fmaf(w4.x, Y[t][4 * q + 0], acc0);
        acc1 = fmaf(w4.y, Y[t][4 * q + 1], acc1);
        acc2 = fmaf(w4.z, Y[t][4 * q + 2], acc2);
        acc3 = fmaf(w4.w, Y[t][4 * q + 3], acc3);
      }
    sigma = (acc0 + acc1) + (acc2 + acc3);
    if constexpr (SAVE) {
      StoreTap<false, kTapBits> tap{srow + TrainSave::off_h(a.n_points, 7), &sb};
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) tap(t, q, Y[t]);
      tap_bits_done(7);
    }
    f32x4 out;
    out.x = 0.0f; out.y = 0.0f; out.z = 0.0f;
    out.w = sigma + __shfl_xor(sigma, 32) + pk[kOffHeadBias + 3];
    if (valid && h == 0) reinterpret_cast<f32x4*>(a.raw)[p] = out;
    return;
  }

  // Layer 7, peeled off the pair loop, and the sigma head on relu(h7) (network.py:61) on a drained ring.  The packed stream
  // ends here for the inference instances: the colour branch reads the FOLD region (nerf_layout.h kFold*), so this GEMM is
  // the last of its stream and must not prefetch past it (the compiler reuses ring registers it believes dead, as in DENS).
  // The training forward still runs the feature layer from the packed stream -- the backward pass needs its row -- so
  // there layer 7 keeps prefetching and the feature GEMM is the last of the stream.
  load_bias<8>(Y, bias + 7 * 256);
  gemm_tiles<8, 8, !SAVE, TrunkTap, kKSkip>(Y, X, ws, save_tap<SAVE, kTapBits>(srow + TrainSave::off_h(a.n_points, 6), &sb), kthr, kpre);
  tap_bits_done(6);
  relu8(Y, 7);
  stream_drain(ws);
  {
    lds_cf32x4* wa = reinterpret_cast<lds_cf32x4*>(tail + (kOffWAlpha - kOffBias) + h * 128);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w4 = wa[t * 4 + q];
        acc0 = fmaf(w4.x, Y[t][4 * q + 0], acc0);
        acc1 = fmaf(w4.y, Y[t][4 * q + 1], acc1);
        acc2 = fmaf(w4.z, Y[t][4 * q + 2], acc2);
        acc3 = fmaf(w4.w, Y[t][4 * q + 3], acc3);
      }
    sigma = (acc0 + acc1) + (acc2 + acc3);
  }
  bool live_tile = true;
  if constexpr (DSKIP) {
    // (wave-uniform) does any point of this tile have sigma > 0?  If none, the colour branch below is skipped as a whole:
    // structured as ONE scalar branch around it that rejoins at the output store -- an early `return` here made the
    // compiler merge the exits behind a divergent store and carry the stream base in VGPRs (not an "s" operand any more)
    const float sigma_full = sigma + __shfl_xor(sigma, 32) + pk[kOffHeadBias + 3];      // the value the tail below writes to out.w
    live_tile = __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(valid && sigma_full > 0.0f) != 0ull)) != 0;
  }

  float rgb[3] = {0.0f, 0.0f, 0.0f};
  if (!DSKIP || live_tile) {
  if constexpr (SAVE) {
    // feature layer (no ReLU, network.py:62): the forward result no longer needs it, the backward pass does (it differentiates
    // the unfolded chain, the same function).  Last GEMM of the packed stream; its row is stored explicitly, as the views row is.
    load_bias<8>(X, bias + 8 * 256);
    gemm_tiles<8, 8, true>(X, Y, ws, save_tap<SAVE, kTapBits>(srow + TrainSave::off_h(a.n_points, 7), &sb));
    tap_bits_done(7);
    StoreTap<false> ftap{srow + TrainSave::off_f(a.n_points), nullptr};
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) ftap(t, q, X[t]);
  }
  // views layer on the folded weights: relu(Wvf . relu(h7) + Wv[:, 256:] . dirs27 + bvf)  ==  network.py:62-67 with
  // feature_linear folded in (nerf_layout.h kFold*).  Every instance, inference or training forward, issues exactly this
  // sequence, so the render under autograd stays bit-equal to the no-grad render.
  f32x16 V[4];
  if (!SAVE) encode_dir();
  wstream_start(ws, reinterpret_cast<const f32x4*>(a.fold + kFoldOffWvf), lane);
  load_bias<4>(V, tail + kTailFloats + h * 64);
  gemm_tiles<8, 4, false, NoTap, kKSkip>(V, Y, ws, NoTap(), kthr);
  gemm_tiles<1, 4, true>(V, DPE, ws);    // last call of the tile: the ring stops at the stream end
  if constexpr (SAVE) {                  // nothing consumes the views row through a GEMM: stored here, as the tile ends
    const u32x4 b = relu_bits_tiles<4>(V);
    if (!NERF_F32_HACK_NOSAVE) bits_out[8 * 64] = b;
    StoreTap<false> tap{a.save + TrainSave::off_hv(a.n_points) + ps * 128 + 4 * h, nullptr};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) tap(t, q, V[t]);
  } else relu_tiles<4>(V);

  // rgb head 128 -> 3 on the VALU (network.py:69)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lds_cf32x4* wr = reinterpret_cast<lds_cf32x4*>(tail + (kOffWRgb - kOffBias) + (c * 2 + h) * 64);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w4 = wr[t * 4 + q];
        acc0 = fmaf(w4.x, V[t][4 * q + 0], acc0);
        acc1 = fmaf(w4.y, V[t][4 * q + 1], acc1);
        acc2 = fmaf(w4.z, V[t][4 * q + 2], acc2);
        acc3 = fmaf(w4.w, V[t][4 * q + 3], acc3);
      }
    rgb[c] = (acc0 + acc1) + (acc2 + acc3);
  }
  // combine the two lane-halves (each holds half of the features of point p)
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] + __shfl_xor(rgb[c], 32) + pk[kOffHeadBias + c];
  }                       // (DSKIP: end of the colour branch; a dead tile arrives here with rgb = 0)
  f32x4 out;
  out.x = rgb[0];
  out.y = rgb[1];
  out.z = rgb[2];
  out.w = sigma + __shfl_xor(sigma, 32) + pk[kOffHeadBias + 3];
  if (valid && h == 0) reinterpret_cast<f32x4*>(a.raw)[p] = out;
  }
}
