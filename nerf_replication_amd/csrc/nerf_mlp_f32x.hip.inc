// "f32x": fp32-accurate fused NeRF MLP on the fp16 matrix cores by operand splitting.
// (same replaced reference lines as nerf_mlp_f32.hip.inc)
//
// Every fp32 operand a is carried as two fp16 numbers, a = a_h + 2^-11 a_l with a_h = fp16(a) and
// a_l = fp16((a - a_h) * 2^11) (exactly representable residual, rescaled into fp16's normal range).
// A product is then   a w = a_h w_h + 2^-11 (a_h w_l + a_l w_h) + O(2^-22 |a w|),
// i.e. THREE v_mfma_f32_32x32x16_f16 with two fp32 accumulators (fp16 x fp16 products are exact in
// fp32) instead of ONE v_mfma_f32_32x32x2_f32 per 8x fewer MACs: 3/16 of the fp32 MFMA cycles at
// ~2^-22 relative operand error (fp32: 2^-24).  Structure follows nerf_mlp_f16.hip.inc (LDS-DMA
// fragment ring with the early barrier, m-outer out-tiles, activations as packed register-resident
// B fragments) with hi and lo copies of everything; 4 waves per workgroup, one per SIMD (the doubled
// activation sets need the whole 512-entry register file), 32 points per wave.

#include "nerf_mlp_common.h"

constexpr int kXStepsPerChunk = nerf::kF16ChunkFrags / 2;                 // 16 (hi, lo) fragment pairs per 32-KiB chunk
constexpr int kXDmaPerWave = nerf::kF16ChunkFrags / kXWaves;              // 8
constexpr int kXPf = 4, kXPfDist = 3;           // (hi, lo) pairs prefetched ahead
constexpr float kXLoScale = 2048.0f, kXLoInv = 1.0f / 2048.0f;
// timing-only experiments (wrong results): where does the matrix pipe wait?
#ifndef NERF_F32X_HACK_NOADV
#define NERF_F32X_HACK_NOADV 0      // never advance the LDS ring (no DMA, no barrier)
#endif
#ifndef NERF_F32X_HACK_NOPE
#define NERF_F32X_HACK_NOPE 0       // positional encodings without sincos
#endif
#ifndef NERF_F32X_HACK_SAVE_NOSTORE
#define NERF_F32X_HACK_SAVE_NOSTORE 0   // training forward without its row stores
#endif
#ifndef NERF_F32X_HACK_NOEPI
#define NERF_F32X_HACK_NOEPI 0      // only the first of the eight epilogue chunks of every tile
#endif

struct XRing {
  const char* gsrc;        // (wave-uniform) byte address of (chunk 0, this wave's first fragment): stays in SGPRs
  unsigned lane_off;       // + this lane's 16 bytes
  lds_char* ldst;
  const lds_char* ring;
  const lds_char* lcur;
  const lds_char* lnext;
  int cur_slot, next_chunk, next_slot;
  int n_chunks;            // stream length in chunks (wrap point)
  int first_chunk;         // chunk the stream wraps back to (0; the density-only backward chain starts behind Wv^T and Wf^T)
  bool dens;               // density-only forward: wrap after the sigma chunk
  h8 pfh[kXPf], pfl[kXPf];
};
// density-only chunk sequence of the forward stream: L0..L7, the sigma chunk (the head's 16 (hi, lo) steps fill exactly one), L0...
constexpr int kXChunkSigma = 2 * nerf::kF16FragSigma / nerf::kF16ChunkFrags;
static_assert((2 * nerf::kF16FragSigma) % nerf::kF16ChunkFrags == 0 && 2 * (nerf::kF16FragFeat - nerf::kF16FragSigma) == nerf::kF16ChunkFrags,
              "the sigma head is one whole chunk");
// the stream wraps after r.n_chunks (kXChunks forward, kXbChunks backward)
__device__ __forceinline__ int xring_next_chunk(const XRing& r) {
  const int nc = r.next_chunk + 1;
  return nc == (r.dens ? kXChunkSigma + 1 : r.n_chunks) ? r.first_chunk : nc;
}
__device__ __forceinline__ void xring_issue(XRing& r) {                       // this wave's 8 DMAs of the next chunk in one burst
  const char* src = r.gsrc + (long long)r.next_chunk * nerf::kF16ChunkBytes;
  lds_char* dst = r.ldst + r.next_slot * nerf::kF16ChunkBytes;
#pragma unroll
  for (int i = 0; i < kXDmaPerWave; ++i)
    __builtin_amdgcn_global_load_lds((gbl_void*)((src + i * nerf::kF16FragBytes) + r.lane_off),
                                     (lds_void*)(dst + i * nerf::kF16FragBytes), 16, 0, 0);
  r.next_chunk = xring_next_chunk(r);
  r.next_slot = (r.next_slot + 1) & (kF16RingSlots - 1);
}
__device__ __forceinline__ void xring_set_slots(XRing& r) {
  r.lcur = r.ring + r.cur_slot * nerf::kF16ChunkBytes;
  r.lnext = r.ring + ((r.cur_slot + 1) & (kF16RingSlots - 1)) * nerf::kF16ChunkBytes;
}
// Ring protocol (4 slots): while chunk c is consumed, chunk c+1 is certified (landed, seen by every wave), chunk c+2
// has been requested a chunk earlier, and the 8 DMAs of chunk c+3 are issued ONE PER K-STEP behind the MFMAs of the
// first 8 steps of chunk c (into the slot chunk c-1 left).  At the end of chunk c, `s_waitcnt vmcnt(8)` leaves only
// those 8 outstanding, so chunk c+2 has landed, and the barrier certifies it.  Issuing the 8 DMAs in one burst at the
// barrier (the first version) kept the wave off the matrix pipe for ~130 cycles per 1536-cycle chunk.
__device__ __forceinline__ void xring_issue_part(XRing& r, int i) {           // DMA i (0..7) of the chunk being requested
  const char* src = r.gsrc + (long long)r.next_chunk * nerf::kF16ChunkBytes;
  lds_char* dst = r.ldst + r.next_slot * nerf::kF16ChunkBytes;
  __builtin_amdgcn_global_load_lds((gbl_void*)((src + i * nerf::kF16FragBytes) + r.lane_off), (lds_void*)(dst + i * nerf::kF16FragBytes), 16, 0, 0);
  if (i == kXDmaPerWave - 1) {
    r.next_chunk = xring_next_chunk(r);
    r.next_slot = (r.next_slot + 1) & (kF16RingSlots - 1);
  }
}
__device__ __forceinline__ void xring_advance(XRing& r) {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  r.cur_slot = (r.cur_slot + 1) & (kF16RingSlots - 1);
  xring_set_slots(r);
}
// after the MFMAs of k-step `fi` of a chunk: this step's share of the DMA traffic, and the chunk boundary
__device__ __forceinline__ void xring_step(XRing& r, int fi) {
  if (fi < kXDmaPerWave) xring_issue_part(r, fi);
  if (fi == kXStepsPerChunk - 1) xring_advance(r);
}
__device__ __forceinline__ void xfrag_read(const XRing& r, int pstep, h8& hi, h8& lo) {   // pstep in [0, 32): static
  const lds_char* base = (pstep < kXStepsPerChunk ? r.lcur : r.lnext) + (pstep & (kXStepsPerChunk - 1)) * (2 * nerf::kF16FragBytes);
  hi = *reinterpret_cast<lds_ch8*>(base);
  lo = *reinterpret_cast<lds_ch8*>(base + nerf::kF16FragBytes);
}

__device__ __forceinline__ void split16(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)((v - (float)hi) * kXLoScale);
}

// ---- LDS reads by inline asm with COUNTED waits (round 3) -------------------------------------------------------------------------
// hipcc turns every `s_waitcnt lgkmcnt` it places in this kernel into lgkmcnt(0): an LDS-DMA (`global_load_lds`) counts as a
// "flat" access for its waitcnt pass, the pass only sees its OWN waits (not the asm `s_waitcnt vmcnt(8)` of the ring protocol), so
// a DMA is "pending" from its point of view for the whole kernel, and with a pending flat access it forces every wait to zero.  A
// full drain in front of an MFMA also waits for the fragment pair that was issued a moment ago, i.e. it exposes one LDS round trip
// (~150 cycles) every 4 k-steps (one wave per SIMD: nobody covers it) -- 236 drains per tile in the ISA of the round-2 kernel.
// So the fragment and bias reads are issued by inline asm (invisible to that pass) and waited for with exact counts: LDS
// operations return in order, and the pair of k-step fi, issued kXPfDist steps earlier, has exactly 2 * kXPfDist younger reads
// behind it (+ 4 when a tile's bias quads were issued in between).  As with the asm global-load rings, no instruction may touch a
// destination register between an asm read and the wait that covers it: tools/check_asm_stream.py proves it on the ISA.

template <int PSTEP>
__device__ __forceinline__ void xfrag_read_asm(const XRing& r, h8& hi, h8& lo) {     // PSTEP in [0, 32)
  const unsigned base = (unsigned)(size_t)(PSTEP < kXStepsPerChunk ? r.lcur : r.lnext);
  asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
               : "=&v"(hi), "=&v"(lo)
               : "v"(base), "n"((PSTEP & (kXStepsPerChunk - 1)) * 2 * nerf::kF16FragBytes),
                 "n"((PSTEP & (kXStepsPerChunk - 1)) * 2 * nerf::kF16FragBytes + nerf::kF16FragBytes));
}
// The bias of the NEXT out-tile: its 16 floats (accumulator-row order) are fetched while the current tile's MFMAs run and become
// the initial value of the next tile's hi accumulator -- no bias registers survive into the epilogue and no add is spent on them.
struct XBias { f32x4 q0, q1, q2, q3; };
__device__ __forceinline__ void xbias_read_asm(lds_cfloat* p, XBias& b) {
  const unsigned a = (unsigned)(size_t)p;
  asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:48"
               : "=&v"(b.q0), "=&v"(b.q1), "=&v"(b.q2), "=&v"(b.q3) : "v"(a));
}
template <int N>
__device__ __forceinline__ void xwait_pair(h8& hi, h8& lo) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(hi), "+v"(lo) : "n"(N));
}
template <int N>
__device__ __forceinline__ void xwait_pair_bias(h8& hi, h8& lo, XBias& b) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(hi), "+v"(lo), "+v"(b.q0), "+v"(b.q1), "+v"(b.q2), "+v"(b.q3) : "n"(N));
}
// every asm read still in flight has landed (tied to all ring registers and the bias quads): before code that does not consume them
// in ring order
__device__ __forceinline__ void xring_drain_reads(XRing& r, XBias& b) {
  static_assert(kXPf == 4, "operand list below");
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r.pfh[0]), "+v"(r.pfh[1]), "+v"(r.pfh[2]), "+v"(r.pfh[3]),
                                        "+v"(r.pfl[0]), "+v"(r.pfl[1]), "+v"(r.pfl[2]), "+v"(r.pfl[3]),
                                        "+v"(b.q0), "+v"(b.q1), "+v"(b.q2), "+v"(b.q3));
}
__device__ __forceinline__ void xbias_read_sync(lds_cfloat* p, XBias& b) {
  const unsigned a = (unsigned)(size_t)p;
  asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\tds_read_b128 %3, %4 offset:48\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(b.q0), "=&v"(b.q1), "=&v"(b.q2), "=&v"(b.q3) : "v"(a));
}
// prime the register prefetch on the first kXPfDist pairs of the chunk being consumed (kernel start, after a skipped colour branch),
// asm reads -- synchronously: reads and their wait in ONE asm statement, for places where the compiler copies registers right
// behind the defining statement (in front of a loop or a join of branches): nothing can come between a read and its wait
__device__ __forceinline__ void xring_prime_sync(XRing& r) {
  static_assert(kXPfDist == 3, "operand list below");
  const unsigned base = (unsigned)(size_t)r.lcur;
  asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %6 offset:1024\n\tds_read_b128 %2, %6 offset:2048\n\t"
               "ds_read_b128 %3, %6 offset:3072\n\tds_read_b128 %4, %6 offset:4096\n\tds_read_b128 %5, %6 offset:5120\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(r.pfh[0]), "=&v"(r.pfl[0]), "=&v"(r.pfh[1]), "=&v"(r.pfl[1]), "=&v"(r.pfh[2]), "=&v"(r.pfl[2]) : "v"(base));
}

// ---- the k-step: the (hi, lo) fragment pair of k-step fi of the chunk sits in ring registers fi % kXPf -----------------------------
// request the pair kXPfDist steps ahead of FI.  ASM: by inline asm, to be waited for with a counted xwait_pair; else an ordinary
// read the compiler schedules (and drains for: the training kernels, see XRowStage below)
template <int FI, bool ASM>
__device__ __forceinline__ void xfrag_prefetch(XRing& r) {
  constexpr int p = FI + kXPfDist;
  if constexpr (ASM) xfrag_read_asm<p>(r, r.pfh[p % kXPf], r.pfl[p % kXPf]);
  else xfrag_read(r, p, r.pfh[p % kXPf], r.pfl[p % kXPf]);
}
// a w = a_h w_h + 2^-11 (a_h w_l + a_l w_h): the three MFMAs of a k-step, A fragments (wh, wl) from the ring, B fragments (bh, bl)
// (operands by value: hipcc simplifies a helper on its own before it inlines it, and one that reaches the ring registers
// through a reference comes out scheduled differently from the same lines written in place -- LAB_NOTEBOOK.md)
__device__ __forceinline__ void xmfma3(f32x16& ah, f32x16& al, h8 wh, h8 wl, h8 bh, h8 bl) {
  ah = mfma16(wh, bh, ah);
  al = mfma16(wh, bl, al);
  al = mfma16(wl, bh, al);
}

// one out-tile without bias (the heads add theirs at the output, the backward chain has none): returns  sum_s W(s) . B[s]  in fp32
// (hi and lo accumulators combined); F0: position of its first k-step in the chunk.  ASM: the inference kernel's asm reads with
// counted waits; else the training kernels' compiler-scheduled reads.
template <int KS1, int KS2, int F0, bool ASM>
__device__ __forceinline__ f32x16 gemmx_tile(XRing& r, const h8* B1h, const h8* B1l, const h8* B2h, const h8* B2l) {
  f32x16 ah, al;
#pragma unroll
  for (int i = 0; i < 16; ++i) { ah[i] = 0.0f; al[i] = 0.0f; }
  static_for<KS1 + KS2>([&](auto S) {
    constexpr int s = decltype(S)::value;
    constexpr int fi = (F0 + s) & (kXStepsPerChunk - 1);
    xfrag_prefetch<fi, ASM>(r);
    if constexpr (ASM) xwait_pair<2 * kXPfDist>(r.pfh[fi % kXPf], r.pfl[fi % kXPf]);
    else __builtin_amdgcn_sched_barrier(0x406);
    xmfma3(ah, al, r.pfh[fi % kXPf], r.pfl[fi % kXPf], s < KS1 ? B1h[s] : B2h[s - KS1], s < KS1 ? B1l[s] : B2l[s - KS1]);
    xring_step(r, fi);
  });
  f32x16 out;
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = fmaf(al[i], kXLoInv, ah[i]);
  return out;
}

// Software-pipelined layer.  With one wave per SIMD nothing else fills the matrix pipe while a finished tile is
// combined, biased, rectified and split into the next layer's B fragments (~120 VALU instructions, a quarter of a
// tile's 48 MFMAs), so that epilogue is cut into eight 2-value chunks and issued behind the MFMAs of the NEXT
// tile's first steps.  Only the last tile of a layer has its epilogue exposed.

// (hi, lo) split of a pair, value by value with split16's roundings -- SCALAR fp32 instructions on purpose: beside MFMAs a packed
// v_pk_{fma,add,mul}_f32 costs a lone wave ~17 cycles of issue against 2 x 4 for the two scalar ones (MI355X_MICROARCH.md, "price
// of one filler beside MFMAs": -2.6 % on the fine launch for the combine alone, interleaved A/B); the residual is fma(-hi, 2^11, 2^11 x) = (x - hi) 2^11 exactly (both products are exact), which
// the compiler turns into one v_fma_mix_f32 on the fp16 half instead of v_cvt_f32_f16 + v_sub + v_mul.
// (2^11 is no inline constant and v_fma_mix_f32 takes no literal: handed over in an SGPR -- as a plain constant hipcc parks it in
// a VGPR for the whole kernel and, under pressure, SPILLS it: a scratch reload with its vmcnt(0) drain in every layer)
__device__ __forceinline__ float xlo_scale_sgpr() {
  float k;
  asm("s_mov_b32 %0, 0x45000000" : "=s"(k));
  return k;
}
__device__ __forceinline__ void xsplit_pair(float x0, float x1, h2& hi, h2& lo) {
  hi = __builtin_convertvector(f32x2{x0, x1}, h2);
  const float k = xlo_scale_sgpr();
  const float r0 = fmaf(-(float)hi[0], k, x0 * kXLoScale), r1 = fmaf(-(float)hi[1], k, x1 * kXLoScale);
  lo = __builtin_convertvector(f32x2{r0, r1}, h2);
}

struct XPending {            // a finished tile whose epilogue has not run yet (forward: its bias is already inside ah)
  f32x16 ah, al;
  h2 part_h[3], part_l[3];   // fp16 pairs of the fragment being assembled (the fourth pair completes it)
};
// the split pair of chunk q joins the B fragment being assembled; every fourth one completes it: k-step 2 mm + (q >> 2) of the
// next GEMM
__device__ __forceinline__ void xpending_emit(XPending& t, int mm, int q, h2 hi, h2 lo, h8* OUTh, h8* OUTl) {
  const int k = q & 3;
  if (k < 3) { t.part_h[k] = hi; t.part_l[k] = lo; }
  else {
    const h4 h01 = __builtin_shufflevector(t.part_h[0], t.part_h[1], 0, 1, 2, 3), h23 = __builtin_shufflevector(t.part_h[2], hi, 0, 1, 2, 3);
    const h4 l01 = __builtin_shufflevector(t.part_l[0], t.part_l[1], 0, 1, 2, 3), l23 = __builtin_shufflevector(t.part_l[2], lo, 0, 1, 2, 3);
    OUTh[2 * mm + (q >> 2)] = __builtin_shufflevector(h01, h23, 0, 1, 2, 3, 4, 5, 6, 7);
    OUTl[2 * mm + (q >> 2)] = __builtin_shufflevector(l01, l23, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

// chunk q (0..7) of the inference epilogue of tile mm: values 2q, 2q+1 -- combine (2 v_fma_f32), ReLU (2 v_max), split
// (xsplit_pair: same roundings as split16 value by value)
__device__ __forceinline__ void xepilogue_chunk(XPending& t, int mm, int q, h8* OUTh, h8* OUTl, bool relu) {
  f32x2 x;                      // (scalar fp32 instructions on purpose: xsplit_pair)
  x.x = fmaf(t.al[2 * q], kXLoInv, t.ah[2 * q]); x.y = fmaf(t.al[2 * q + 1], kXLoInv, t.ah[2 * q + 1]);
  if (relu) x = __builtin_elementwise_max(x, f32x2{0.0f, 0.0f});
  h2 hi, lo;
  xsplit_pair(x.x, x.y, hi, lo);
  xpending_emit(t, mm, q, hi, lo, OUTh, OUTl);
}

// The inference layer (asm reads with counted waits).
// (Carrying a layer's last pending tile into the next layer's first tile was tried: +0.6 %, not kept.)
// `nb` enters holding (in flight or landed) the bias of this layer's out-tile 0 and leaves holding that of the layer that follows
// (next_layer_bias, with HAS_NEXT; without: nothing is fetched and nb is left dead).
template <int KS1, int KS2, int NM, int F0, bool HAS_NEXT>
__device__ __forceinline__ void gemmx_layer(XRing& r, XBias& nb, lds_cfloat* bias_lds_h, lds_cfloat* next_layer_bias,
                                            const h8* B1h, const h8* B1l, const h8* B2h, const h8* B2l, h8* OUTh, h8* OUTl,
                                            bool relu) {
  constexpr int KS = KS1 + KS2;
  constexpr int kCps = (8 + KS - 1) / KS;                 // epilogue chunks issued per k-step
  constexpr int kBiasAt = KS - 3;                         // k-step at which the NEXT tile's bias is requested (waited for one step later)
  static_assert(kBiasAt >= 1, "the current tile consumes nb at k-step 0");
  XPending pend;
  static_for<NM>([&](auto M) {
    constexpr int m = decltype(M)::value;
    XPending cur;
    constexpr bool fetch_next = (m + 1 < NM) || HAS_NEXT;          // (an LDS address can be 0: the flag is a template argument)
    static_for<KS>([&](auto S) {
      constexpr int s = decltype(S)::value;
      constexpr int fi = (F0 + m * KS + s) & (kXStepsPerChunk - 1);
      // LDS operations of a k-step, in program order (all inline asm, so the order is fixed): [the next tile's 4 bias reads at
      // k-step kBiasAt], then the fragment pair of k-step fi + kXPfDist.  The pair of k-step fi has 2 * kXPfDist younger fragment
      // reads behind it (+ 4 at k-step kBiasAt itself); one step later the wait is tightened to "only the two newest pairs may be
      // outstanding", which covers the bias quads (tied there; the pair it additionally waits for was issued two steps ago).
      if constexpr (s == kBiasAt && fetch_next) xbias_read_asm(m + 1 < NM ? bias_lds_h + (m + 1) * 16 : next_layer_bias, nb);
      xfrag_prefetch<fi, true>(r);
      if constexpr (s == kBiasAt && fetch_next) xwait_pair<2 * kXPfDist + 4>(r.pfh[fi % kXPf], r.pfl[fi % kXPf]);
      else if constexpr (s == kBiasAt + 1 && fetch_next) xwait_pair_bias<4>(r.pfh[fi % kXPf], r.pfl[fi % kXPf], nb);
      else xwait_pair<2 * kXPfDist>(r.pfh[fi % kXPf], r.pfl[fi % kXPf]);
      if constexpr (s == 0) {                               // the accumulator starts from the tile's bias (landed and tied a tile ago)
        cur.ah[0] = nb.q0.x; cur.ah[1] = nb.q0.y; cur.ah[2] = nb.q0.z; cur.ah[3] = nb.q0.w;
        cur.ah[4] = nb.q1.x; cur.ah[5] = nb.q1.y; cur.ah[6] = nb.q1.z; cur.ah[7] = nb.q1.w;
        cur.ah[8] = nb.q2.x; cur.ah[9] = nb.q2.y; cur.ah[10] = nb.q2.z; cur.ah[11] = nb.q2.w;
        cur.ah[12] = nb.q3.x; cur.ah[13] = nb.q3.y; cur.ah[14] = nb.q3.z; cur.ah[15] = nb.q3.w;
#pragma unroll
        for (int i = 0; i < 16; ++i) cur.al[i] = 0.0f;
      }
      xmfma3(cur.ah, cur.al, r.pfh[fi % kXPf], r.pfl[fi % kXPf], s < KS1 ? B1h[s] : B2h[s - KS1], s < KS1 ? B1l[s] : B2l[s - KS1]);
      if constexpr (m > 0) {
#pragma unroll
        for (int c = 0; c < kCps; ++c)
          if (s * kCps + c < (NERF_F32X_HACK_NOEPI ? 1 : 8)) xepilogue_chunk(pend, m - 1, s * kCps + c, OUTh, OUTl, relu);
      }
      if (!NERF_F32X_HACK_NOADV) xring_step(r, fi);
    });
    pend = cur;
  });
#pragma unroll
  for (int q = 0; q < (NERF_F32X_HACK_NOEPI ? 1 : 8); ++q) xepilogue_chunk(pend, NM - 1, q, OUTh, OUTl, relu);
}

// ---- the training kernels' layer (SAVE forward here, backward chain in nerf_mlp_bwd_f32x.hip.inc): compiler-scheduled LDS reads
// (every wait hipcc places is a full drain, see above; with 256 + 256 registers in use it parks freshly "read" asm fragments in
// AGPRs before they have landed: 14 hazards in tools/check_asm_stream.py), software-pipelined like the inference layer.
// Every store is UNCONDITIONAL: the lanes of a ragged last tile write their (duplicate) rows into the pad32 padding of the
// TrainSave regions, and a wave without a 32-point tile never gets here (it lets the whole stream go by) -- round 2 predicated
// each of the ~250 row stores of a tile with its own s_and_saveexec / s_cbranch_execz.
// Row stores through a per-wave LDS transpose (round 3).  In the accumulator layout lane (p, h) holds 4 consecutive features of
// ROW p, so a direct `global_store_dwordx4` writes 64 separate 16-byte pieces (rows are 1 KiB apart, and the two halves of a
// row's 32 bytes sit in lanes p and p + 32): the SAVE forward and the chain ran at ~2 TB/s of stores, and without their stores
// they were 23 % / 48 % faster.  Each finished 32 x 32 tile (4 KiB) therefore goes through the 4 KiB of LDS the weight ring
// leaves per wave: 4 ds_write_b128 in accumulator layout, 4 ds_read_b128 with lanes 8r..8r+7 on the eight 16-byte pieces of ONE
// row, so every global store writes 8 full 128-byte lines.  16-byte piece c of row p lives at p * 128 + (c ^ (p & 7)) * 16:
// conflict-free for the 8-lane groups of ds_write_b128 (32 banks) and the 16-lane groups of ds_read_b128 (64 banks)
// (MI355X_MICROARCH.md, LDS table).  LDS operations of a wave execute in order, so the reads need no wait for the writes.
constexpr int kXStageBytes = 4096;                       // per wave
struct XRowStage {
  unsigned w0;             // this lane's write address for quad 0: buf + p * 128 + ((h ^ (p & 1)) + ((p & 7) >> 1) * 2) * 16
  unsigned r0;             // this lane's read address: buf + (l >> 3) * 128 + ((l & 7) ^ (l >> 3)) * 16
  unsigned goff256, goff128;   // byte offset of (row l >> 3, piece l & 7) in a row-major tile with 1-KiB / 512-byte rows
};
__device__ __forceinline__ XRowStage xstage_init(lds_char* buf, int lane) {
  const unsigned p = lane & 31, h = lane >> 5, l = lane;
  XRowStage st;
  st.w0 = (unsigned)(size_t)buf + p * 128u + ((h ^ (p & 1u)) + ((p & 7u) >> 1) * 2u) * 16u;
  st.r0 = (unsigned)(size_t)buf + (l >> 3) * 128u + ((l & 7u) ^ (l >> 3)) * 16u;
  st.goff256 = (l >> 3) * 1024u + (l & 7u) * 16u;
  st.goff128 = (l >> 3) * 512u + (l & 7u) * 16u;
  return st;
}
// quad q (0..3) of this lane's row: features 8 q + 4 h .. + 3 of the tile (the buffer is 128-byte aligned, so piece bits 1..2 of
// the address are `q ^ ((p & 7) >> 1)` = the address of quad 0 with q xor-ed in)
template <int Q4>
__device__ __forceinline__ void xstage_put(const XRowStage& st, const f32x4& v) {
  *reinterpret_cast<lds_f32x4*>(st.w0 ^ (unsigned)(Q4 * 32)) = v;
}
// the transposed tile comes back in two halves (rows 0..15, 16..31: two 16-byte quads per lane each) to keep the registers few
struct XStaged { f32x4 v[2]; };
template <int HALF>
__device__ __forceinline__ void xstage_get(const XRowStage& st, XStaged& g) {
#pragma unroll
  for (int i = 0; i < 2; ++i) g.v[i] = *reinterpret_cast<lds_cf32x4*>(st.r0 + (2 * HALF + i) * 1024);
}
// `tile_rows`: wave-uniform address of feature 0 of the tile's row 0 in a row-major region with ROWB-byte rows; m: out-tile
template <int ROWB, int HALF>
__device__ __forceinline__ void xstage_store(const XRowStage& st, const XStaged& g, float* tile_rows, int m) {
  char* base = reinterpret_cast<char*>(tile_rows) + (ROWB == 1024 ? st.goff256 : st.goff128) + m * 128;
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(base + (2 * HALF + i) * 8 * ROWB) = g.v[i];
}
// the whole round trip of one tile in place (where no later k-step of the layer is left to spread it over)
template <int ROWB>
__device__ __forceinline__ void xstage_flush(const XRowStage& st, float* tile_rows, int m) {
  XStaged g;
  xstage_get<0>(st, g); xstage_store<ROWB, 0>(st, g, tile_rows, m);
  xstage_get<1>(st, g); xstage_store<ROWB, 1>(st, g, tile_rows, m);
}

// The layer skeleton of both training kernels: NM out-tiles of KS1 + KS2 k-steps (B1 then B2 fragments; F0: position of the first
// k-step in the chunk).  `init(cur, M)` starts tile M's accumulators, `chunk(pend, MM, Q)` is chunk Q (0..7) of the epilogue of
// the finished tile MM (M, MM, Q: std::integral_constant) -- issued kCps per k-step behind the MFMAs of the NEXT tile, only the
// layer's last tile has its epilogue exposed.  STAGE_IO: the chunks write the tile's quads to the LDS stage (xstage_put, every
// second chunk one), the transposed halves come back in the two k-steps behind chunk 7 and are stored one k-step after their
// read (`tile_rows`: wave-uniform address of (row 0, feature 0) of this wave's 32-point tile in the layer's row-major region with
// ROWB-byte rows); where no k-step is left to spread that over, and for the last tile, the round trip runs in place.
template <int KS1, int KS2, int NM, int F0, int ROWB, bool STAGE_IO, class Init, class Chunk>
__device__ __forceinline__ void gemmx_layer_train(XRing& r, const h8* B1h, const h8* B1l, const h8* B2h, const h8* B2l,
                                                  const XRowStage& st, float* tile_rows, Init&& init, Chunk&& chunk) {
  constexpr int KS = KS1 + KS2;
  constexpr int kCps = (8 + KS - 1) / KS;                 // epilogue chunks issued per k-step
  constexpr int kS7 = 7 / kCps;                           // k-step that issues chunk 7
  constexpr bool kLate = kS7 + 2 < KS;                    // stage reads / stores spread over the k-steps behind chunk 7 (else: in place)
  XStaged stg;
  XPending pend;
  static_for<NM>([&](auto M) {
    constexpr int m = decltype(M)::value;
    XPending cur;
    init(cur, M);
    static_for<KS>([&](auto S) {
      constexpr int s = decltype(S)::value;
      constexpr int fi = (F0 + m * KS + s) & (kXStepsPerChunk - 1);
      xfrag_prefetch<fi, false>(r);
      __builtin_amdgcn_sched_barrier(0x406);
      xmfma3(cur.ah, cur.al, r.pfh[fi % kXPf], r.pfl[fi % kXPf], s < KS1 ? B1h[s] : B2h[s - KS1], s < KS1 ? B1l[s] : B2l[s - KS1]);
      if constexpr (m > 0) {
        static_for<kCps>([&](auto C) {
          constexpr int q = s * kCps + decltype(C)::value;
          if constexpr (q < 8) chunk(pend, std::integral_constant<int, m - 1>{}, std::integral_constant<int, q>{});
        });
        if constexpr (STAGE_IO) {
          if constexpr (kLate) {
            if constexpr (s == kS7) xstage_get<0>(st, stg);
            if constexpr (s == kS7 + 1) { xstage_store<ROWB, 0>(st, stg, tile_rows, m - 1); xstage_get<1>(st, stg); }
            if constexpr (s == kS7 + 2) xstage_store<ROWB, 1>(st, stg, tile_rows, m - 1);
          } else if constexpr (s == kS7) xstage_flush<ROWB>(st, tile_rows, m - 1);
        }
      }
      xring_step(r, fi);
    });
    pend = cur;
  });
  static_for<8>([&](auto Q) { chunk(pend, std::integral_constant<int, NM - 1>{}, Q); });
  if constexpr (STAGE_IO) xstage_flush<ROWB>(st, tile_rows, NM - 1);
}

struct XSaveBits { unsigned w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u; };      // (scalars: stay in registers)

// chunk Q (0..7) of the SAVE forward's epilogue of tile MM: values 2Q, 2Q+1 -- combine, ReLU on the bit pattern (2 v_max_i32), split
// (xsplit_pair: same roundings as split16 value by value); every second chunk writes one 16-byte quad of this lane's row to the
// LDS stage.  BITS: the ReLU sign bits of this lane's values in the layout of the fp32 SAVE forward (TrainSave::off_bits: bit
// 16 (MM & 1) + r of word MM >> 1 <-> accumulator register r of out-tile MM; the C/D layout of the 32x32 MFMAs is
// dtype-independent): a rectified value is a non-negative integer, so "> 0" is min(bits, 1) -- v_min_u32 + v_lshl_or_b32 per value.
template <bool RELU, bool BITS, int MM, int Q>
__device__ __forceinline__ void xepilogue_chunk_s(XPending& t, h8* OUTh, h8* OUTl, const XRowStage& st, float (&keep)[2], XSaveBits& sb) {
  f32x2 x;                      // (scalar fp32 instructions on purpose: xsplit_pair)
  x.x = fmaf(t.al[2 * Q], kXLoInv, t.ah[2 * Q]); x.y = fmaf(t.al[2 * Q + 1], kXLoInv, t.ah[2 * Q + 1]);
  if constexpr (RELU) {
    const int i0 = max(__float_as_int(x.x), 0), i1 = max(__float_as_int(x.y), 0);
    x.x = __int_as_float(i0); x.y = __int_as_float(i1);
    if constexpr (BITS) {
      // (hipcc turns min(v, 1) into compare + select and splits the shift from the or: asm keeps it at two VALU per value)
      auto put = [&](unsigned& w) {
        unsigned t0, t1;
        asm("v_min_u32 %0, 1, %1" : "=v"(t0) : "v"(i0));
        asm("v_min_u32 %0, 1, %1" : "=v"(t1) : "v"(i1));
        asm("v_lshl_or_b32 %0, %1, %2, %0" : "+v"(w) : "v"(t0), "n"(16 * (MM & 1) + 2 * Q));
        asm("v_lshl_or_b32 %0, %1, %2, %0" : "+v"(w) : "v"(t1), "n"(16 * (MM & 1) + 2 * Q + 1));
      };
      if constexpr ((MM >> 1) == 0) put(sb.w0); else if constexpr ((MM >> 1) == 1) put(sb.w1);
      else if constexpr ((MM >> 1) == 2) put(sb.w2); else put(sb.w3);
    }
  }
  h2 hi, lo;
  xsplit_pair(x.x, x.y, hi, lo);
  xpending_emit(t, MM, Q, hi, lo, OUTh, OUTl);
  if (Q & 1) {
    f32x4 o4; o4.x = keep[0]; o4.y = keep[1]; o4.z = x.x; o4.w = x.y;
    if constexpr (!NERF_F32X_HACK_SAVE_NOSTORE) xstage_put<(Q >> 1)>(st, o4);
  } else { keep[0] = x.x; keep[1] = x.y; }
}

// The SAVE forward's layer: the bias (16 floats per out-tile, accumulator-row order) is the hi accumulator's initial value; the
// post-activation rows go through the LDS stage to `tile_rows`, the sign-bit words of a rectified layer to `bits_dst`.  (The
// unnamed pointer is this lane's own row, which nothing stores to any more: the caller says why it is still computed.)
template <int KS1, int KS2, int NM, int F0, bool RELU, bool BITS, int ROWB>
__device__ __forceinline__ void gemmx_layer_s(XRing& r, lds_cfloat* bias_lds_h, const h8* B1h, const h8* B1l,
                                              const h8* B2h, const h8* B2l, h8* OUTh, h8* OUTl,
                                              float* __restrict__ /*row*/, const XRowStage& st, float* tile_rows,
                                              unsigned* __restrict__ bits_dst) {
  static_assert(!BITS || RELU, "sign bits belong to rectified layers");
  XSaveBits sb;
  float keep[2] = {0.0f, 0.0f};
  gemmx_layer_train<KS1, KS2, NM, F0, ROWB, !NERF_F32X_HACK_SAVE_NOSTORE>(r, B1h, B1l, B2h, B2l, st, tile_rows,
    [&](XPending& cur, auto M) {
#pragma unroll
      for (int i = 0; i < 16; ++i) cur.al[i] = 0.0f;
      lds_cf32x4* b = reinterpret_cast<lds_cf32x4*>(bias_lds_h + decltype(M)::value * 16);
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 bq = b[q4];
        cur.ah[4 * q4 + 0] = bq.x; cur.ah[4 * q4 + 1] = bq.y; cur.ah[4 * q4 + 2] = bq.z; cur.ah[4 * q4 + 3] = bq.w;
      }
    },
    [&](XPending& t, auto MM, auto Q) {
      xepilogue_chunk_s<RELU, BITS, decltype(MM)::value, decltype(Q)::value>(t, OUTh, OUTl, st, keep, sb);
    });
  if constexpr (BITS) {                                     // one coalesced 1-KiB block per wave and layer
    u32x4 w; w.x = sb.w0; w.y = sb.w1; w.z = sb.w2; w.w = sb.w3;
    *reinterpret_cast<u32x4*>(bits_dst) = w;
  }
}

// DENS: stop after the sigma head (MlpArgs::density_only), raw = (0, 0, 0, sigma).  DSKIP (MlpArgs::skip_dead_colour): a wave whose 32
// points all have sigma <= 0 lets the colour branch's 13 chunks go by unread (it still issues its DMA share and meets the
// chunk barriers) and writes rgb = 0 -- as nerf_mlp_f16_kernel does.
template <bool RAY_MODE, bool SAVE = false, bool DENS = false, bool DSKIP = false>
__global__ __launch_bounds__(kXThreads) __attribute__((amdgpu_waves_per_eu(1, 1)))
void nerf_mlp_f32x_kernel(MlpArgs a) {
  static_assert(!(DSKIP && DENS), "dead-colour skipping is a variant of the full network");
  using namespace nerf;
  // (training forward: + 4 KiB per wave for the row-store transpose, XRowStage -- exactly what the weight ring leaves of the 160 KiB)
  __shared__ __attribute__((aligned(128))) char smem_generic[kF16LdsBytes + (SAVE ? kXWaves * kXStageBytes : 0)];
  lds_char* smem = (lds_char*)smem_generic;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5;
  const char* packed = reinterpret_cast<const char*>(a.packed);
  if (a.index && *a.count <= 0) return;
  const XRowStage st = xstage_init(smem + kF16LdsBytes + (SAVE ? wave * kXStageBytes : 0), lane);
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
  r.cur_slot = 0; r.next_chunk = 0; r.next_slot = 0; r.n_chunks = kXChunks; r.first_chunk = 0; r.dens = DENS;
  xring_issue(r); xring_issue(r); xring_issue(r);
  asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");      // const region + chunks 0, 1 landed
  __builtin_amdgcn_sched_barrier(0);
  xring_set_slots(r);
  lds_cfloat* cst = reinterpret_cast<lds_cfloat*>(smem);
  lds_cfloat* bias_h = cst + kF16OffBias + h * 128;
  lds_cfloat* bias_views_h = cst + kF16OffBiasViews + h * 64;
  // the four head biases once, BEFORE any asm read is in flight (a compiler-placed LDS read inside the tile loop would be waited for
  // with a full drain, and would not be counted by the asm waits)
  const float hb_r = cst[kF16OffHeadBias + 0], hb_g = cst[kF16OffHeadBias + 1], hb_b = cst[kF16OffHeadBias + 2], hb_s = cst[kF16OffHeadBias + 3];
  float hb_sink = hb_r + hb_g + hb_b + hb_s;
  asm volatile("" : "+v"(hb_sink));                                     // (the values are in registers here: their reads have been waited for)
  XBias nb;
  if constexpr (SAVE) {
#pragma unroll
    for (int i = 0; i < kXPfDist; ++i) xfrag_read(r, i, r.pfh[i], r.pfl[i]);
  } else {
    xring_prime_sync(r);                 // (in front of the loop: the compiler copies into the loop-carried registers right here)
    xbias_read_sync(bias_h, nb);
  }

  const long long n_points = a.index ? (long long)*a.count : a.n_points;
  const long long n_tiles = (n_points + kXTilePts - 1) / kXTilePts;
  // a wave lets `n` chunks of the stream go by unread: it still issues its share of the DMAs and meets the chunk barriers
  auto skip_chunks = [&](int n) {
#pragma unroll 1
    for (int c = 0; c < n; ++c) {
#pragma unroll
      for (int i = 0; i < kXDmaPerWave; ++i) xring_issue_part(r, i);
      xring_advance(r);
    }
  };
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    long long pl = tile * kXTilePts + wave * 32 + (lane & 31);
    // training forward: every store of a tile is unconditional -- lanes past the last point write their (duplicate) rows into the
    // pad32 padding of the TrainSave regions at their OWN row index `prow`; a wave whose 32-point tile does not exist at all
    // (ragged last 128-point tile) lets the whole stream go by
    const long long prow = pl;
    if constexpr (SAVE) {
      if ((tile * kXWaves + wave) * 32 >= TrainSave::pad32(n_points)) {                    // (wave-uniform)
        skip_chunks(DENS ? kXChunkSigma + 1 : kXChunks);
#pragma unroll
        for (int i = 0; i < kXPfDist; ++i) xfrag_read(r, i, r.pfh[i], r.pfl[i]);
        continue;
      }
    }
    const bool valid = pl < n_points;
    if (!valid) pl = n_points - 1;
    const long long p = a.index ? (long long)a.index[pl] : pl;
    const long long ray = p / a.n_samples;
    const int s_idx = (int)(p - ray * a.n_samples);
    float x[3], d[3];
    if (RAY_MODE) {
      const float t = a.tvals[ray * a.t_ray_stride + s_idx];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        d[c] = a.rays_d[ray * 3 + c];
        x[c] = __fadd_rn(a.rays_o[ray * 3 + c], __fmul_rn(d[c], t));
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = a.pts[p * 3 + c];
    }
    if (a.viewdirs != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] = a.viewdirs[ray * 3 + c];
    } else {
      const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] = __fdiv_rn(d[c], nrm);
    }
    // positional encodings (fp32-accurate: every octave by its own Cody-Waite sincos), split into hi / lo fragments
    h8 PEh[4], PEl[4], DPEh[2], DPEl[2];
    {
      const float hs = h ? 32.0f : 1.0f;
#pragma unroll
      for (int ai = 0; ai < 15; ++ai) {
        float sv, cv;
        if (NERF_F32X_HACK_NOPE) { sv = x[ai % 3] * hs; cv = sv * 0.5f; } else sincos_cw(x[ai % 3] * (hs * (float)(1 << (ai / 3))), sv, cv);
        if (SAVE) {
          float* pe_row = a.save + TrainSave::off_pe(a.n_points) + prow * 64;
          pe_row[h ? pe_xyz_feat(2 * ai, 1) : pe_xyz_feat(2 * ai, 0)] = sv;
          pe_row[h ? pe_xyz_feat(2 * ai + 1, 1) : pe_xyz_feat(2 * ai + 1, 0)] = cv;
        }
        _Float16 th, tl;
        split16(sv, th, tl); PEh[(2 * ai) >> 3][(2 * ai) & 7] = th; PEl[(2 * ai) >> 3][(2 * ai) & 7] = tl;
        split16(cv, th, tl); PEh[(2 * ai + 1) >> 3][(2 * ai + 1) & 7] = th; PEl[(2 * ai + 1) >> 3][(2 * ai + 1) & 7] = tl;
      }
      if (SAVE) {
        float* pe_row = a.save + TrainSave::off_pe(a.n_points) + prow * 64;
        if (h) { pe_row[2] = x[2]; pe_row[63] = 0.0f; } else { pe_row[0] = x[0]; pe_row[1] = x[1]; }
      }
      _Float16 th, tl;
      split16(h ? x[2] : x[0], th, tl); PEh[3][6] = th; PEl[3][6] = tl;
      split16(h ? 0.0f : x[1], th, tl); PEh[3][7] = th; PEl[3][7] = tl;
    }
    // direction encoding: the inference instances build it here; the training forward in front of the views layer, where the h7
    // fragments are dead (16 registers less across the trunk, and waves that skip the colour branch never need it)
    auto make_dpe = [&]() {
      _Float16 th, tl;
      const float ds = h ? 4.0f : 1.0f;
#pragma unroll
      for (int ai = 0; ai < 6; ++ai) {
        float sv, cv;
        if (NERF_F32X_HACK_NOPE) { sv = d[ai % 3] * ds; cv = sv * 0.5f; } else sincos_cw(d[ai % 3] * (ds * (float)(1 << (ai / 3))), sv, cv);
        if (SAVE && !DENS) {
          float* dpe_row = a.save + TrainSave::off_dpe(a.n_points) + prow * 32;
          dpe_row[h ? pe_dir_feat(2 * ai, 1) : pe_dir_feat(2 * ai, 0)] = sv;
          dpe_row[h ? pe_dir_feat(2 * ai + 1, 1) : pe_dir_feat(2 * ai + 1, 0)] = cv;
        }
        split16(sv, th, tl); DPEh[(2 * ai) >> 3][(2 * ai) & 7] = th; DPEl[(2 * ai) >> 3][(2 * ai) & 7] = tl;
        split16(cv, th, tl); DPEh[(2 * ai + 1) >> 3][(2 * ai + 1) & 7] = th; DPEl[(2 * ai + 1) >> 3][(2 * ai + 1) & 7] = tl;
      }
      if (SAVE && !DENS) {
        float* dpe_row = a.save + TrainSave::off_dpe(a.n_points) + prow * 32;
        if (h) { dpe_row[2] = d[2]; dpe_row[27] = 0.f; dpe_row[28] = 0.f; dpe_row[29] = 0.f; dpe_row[30] = 0.f; dpe_row[31] = 0.f; }
        else { dpe_row[0] = d[0]; dpe_row[1] = d[1]; }
      }
      split16(h ? d[2] : d[0], th, tl); DPEh[1][4] = th; DPEl[1][4] = tl;
      split16(h ? 0.0f : d[1], th, tl); DPEh[1][5] = th; DPEl[1][5] = tl;
      DPEh[1][6] = (_Float16)0.0f; DPEl[1][6] = (_Float16)0.0f; DPEh[1][7] = (_Float16)0.0f; DPEl[1][7] = (_Float16)0.0f;
    };
    if constexpr (!SAVE) make_dpe();

    const long long P = a.n_points;
    // feature (8 chunks) + views and rgb (5 chunks): what a wave without density lets go by unread
    constexpr int kColourChunks = 2 * (nerf::kF16Frags - nerf::kF16FragFeat) / nerf::kF16ChunkFrags;
    static_assert(2 * (nerf::kF16Frags - nerf::kF16FragFeat) % nerf::kF16ChunkFrags == 0, "the colour branch is whole chunks");
    h8 Xh[16], Xl[16], Yh[16], Yl[16];
    f32x16 sig, col;
    bool dead_wave = false;                                                                    // (wave-uniform)
    if constexpr (SAVE) {
      // training forward (gemmx_layer_s): every layer's post-activation output also goes to the row-major activation store through
      // the LDS transpose (XRowStage, as in the backward chain), the ReLU sign bits of this wave's 32 points to block
      // (tile * 4 + wave) of the TrainSave bit blocks.  With the MFMA accumulators in VGPRs (this unit's XFLAGS) all instances fit
      // the register file (12 bytes of scratch, touched at the tile boundaries); with hipcc's default allocation only the
      // density-only instance did (LAB_NOTEBOOK.md A9, A10).
      const long long tile32 = tile * kXWaves + wave;
      // this lane's row (+ 4 h) in a row-major region, as (wave-uniform 64-bit base) + (32-bit lane offset).  Nothing stores through
      // it since every row goes through the LDS stage, but the opaque redefinition of its lane offset still shapes the register
      // allocation of the four SAVE instances: taking it out changes their code, so that is a performance change to be measured.
      const unsigned lrow = (unsigned)(wave * 32 + (lane & 31));          // this lane's row inside the 128-point tile
      auto srow = [&](long long off, int width) -> float* {
        const char* base = reinterpret_cast<const char*>(a.save + off + tile * (long long)(kXTilePts * width));
        unsigned lo = lrow;
        asm volatile("" : "+v"(lo));
        return reinterpret_cast<float*>(const_cast<char*>(base) + (lo * (unsigned)(width * 4) + (unsigned)(h * 16)));
      };
      // wave-uniform address of (row 0, feature 0) of this wave's 32-point tile in a row-major region (staged layers)
      auto trow = [&](long long off, int width) -> float* {
        return a.save + off + (tile * (long long)kXTilePts + wave * 32) * width;
      };
      // the bit blocks as (wave-uniform 64-bit base) + (32-bit lane offset): the stores take the base from SGPRs.  (The opaque
      // redefinition of the lane offset keeps the compiler from computing all nine pointers at the top of the tile and spilling them:
      // each is built where its layer starts)
      auto bdst = [&](int which) -> unsigned* {
        const char* base = reinterpret_cast<const char*>(a.save + TrainSave::off_bits(P) + TrainSave::bits_block(tile32, which));
        unsigned lo = (unsigned)lane;
        asm volatile("" : "+v"(lo));
        return reinterpret_cast<unsigned*>(const_cast<char*>(base) + lo * 16u);
      };
      gemmx_layer_s<4, 0, 8, 0, true, true, 1024>(r, bias_h, PEh, PEl, PEh, PEl, Xh, Xl, srow(TrainSave::off_h(P, 0), 256), st, trow(TrainSave::off_h(P, 0), 256), bdst(0));   // L0
#pragma unroll 1
      for (int it = 0; it < 2; ++it) {                                                          // L1..L4
        gemmx_layer_s<16, 0, 8, 0, true, true, 1024>(r, bias_h + (1 + 2 * it) * 256, Xh, Xl, Xh, Xl, Yh, Yl, srow(TrainSave::off_h(P, 1 + 2 * it), 256), st, trow(TrainSave::off_h(P, 1 + 2 * it), 256), bdst(1 + 2 * it));
        gemmx_layer_s<16, 0, 8, 0, true, true, 1024>(r, bias_h + (2 + 2 * it) * 256, Yh, Yl, Yh, Yl, Xh, Xl, srow(TrainSave::off_h(P, 2 + 2 * it), 256), st, trow(TrainSave::off_h(P, 2 + 2 * it), 256), bdst(2 + 2 * it));
      }
      gemmx_layer_s<4, 16, 8, 0, true, true, 1024>(r, bias_h + 5 * 256, PEh, PEl, Xh, Xl, Yh, Yl, srow(TrainSave::off_h(P, 5), 256), st, trow(TrainSave::off_h(P, 5), 256), bdst(5));   // L5 = skip(PE) + hidden
      gemmx_layer_s<16, 0, 8, 0, true, true, 1024>(r, bias_h + 6 * 256, Yh, Yl, Yh, Yl, Xh, Xl, srow(TrainSave::off_h(P, 6), 256), st, trow(TrainSave::off_h(P, 6), 256), bdst(6));     // L6
      gemmx_layer_s<16, 0, 8, 0, true, true, 1024>(r, bias_h + 7 * 256, Xh, Xl, Xh, Xl, Yh, Yl, srow(TrainSave::off_h(P, 7), 256), st, trow(TrainSave::off_h(P, 7), 256), bdst(7));     // L7 -> Y = relu(h7)
      sig = gemmx_tile<16, 0, 0, false>(r, Yh, Yl, Yh, Yl);                                     // sigma head (ahead of the feature layer)
      if constexpr (DSKIP)
        dead_wave = __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(
                        h == 0 && valid && sig[0] + hb_s > 0.0f) != 0ull)) == 0;
      if constexpr (DENS) {
        // density only (coarse pass of a training step: the loss reads the coarse network through the sample positions alone,
        // SURVEY F10): the stream wraps after the sigma chunk; no colour-branch row is stored (the backward never reads one)
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i] = 0.0f;
      } else if (dead_wave) {
        // no density in this wave's 32 points: compositing's adjoint hands the tile a zero gradient, the backward works on live
        // tiles only -- feature / views rows and the views bits are not stored, the colour branch's 13 chunks go by unread
        skip_chunks(kColourChunks);
#pragma unroll
        for (int i = 0; i < kXPfDist; ++i) xfrag_read(r, i, r.pfh[i], r.pfl[i]);
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i] = 0.0f;
      } else {
        gemmx_layer_s<16, 0, 8, 0, false, false, 1024>(r, bias_h + 8 * 256, Yh, Yl, Yh, Yl, Xh, Xl, srow(TrainSave::off_f(P), 256), st, trow(TrainSave::off_f(P), 256), nullptr);       // feature
        make_dpe();
        h8 Vh[8], Vl[8];
        gemmx_layer_s<16, 2, 4, 0, true, true, 512>(r, bias_views_h, Xh, Xl, DPEh, DPEl, Vh, Vl, srow(TrainSave::off_hv(P), 128), st, trow(TrainSave::off_hv(P), 128), bdst(8));       // views
        col = gemmx_tile<8, 0, 8, false>(r, Vh, Vl, Vh, Vl);                                      // rgb head
      }
    } else {
    // inference: LDS reads by inline asm with counted waits.  Entering a tile, every asm read issued so far has landed (the drains at
    // the end of the previous tile's branches / before the loop) and nb holds the bias of (L0, out-tile 0).
    gemmx_layer<4, 0, 8, 0, true>(r, nb, bias_h, bias_h + 256, PEh, PEl, PEh, PEl, Xh, Xl, true);   // L0
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {                                                          // L1..L4
      gemmx_layer<16, 0, 8, 0, true>(r, nb, bias_h + (1 + 2 * it) * 256, bias_h + (2 + 2 * it) * 256, Xh, Xl, Xh, Xl, Yh, Yl, true);
      gemmx_layer<16, 0, 8, 0, true>(r, nb, bias_h + (2 + 2 * it) * 256, bias_h + (3 + 2 * it) * 256, Yh, Yl, Yh, Yl, Xh, Xl, true);
    }
    gemmx_layer<4, 16, 8, 0, true>(r, nb, bias_h + 5 * 256, bias_h + 6 * 256, PEh, PEl, Xh, Xl, Yh, Yl, true);   // L5 = skip(PE) + hidden
    gemmx_layer<16, 0, 8, 0, true>(r, nb, bias_h + 6 * 256, bias_h + 7 * 256, Yh, Yl, Yh, Yl, Xh, Xl, true);     // L6
    gemmx_layer<16, 0, 8, 0, !DENS>(r, nb, bias_h + 7 * 256, bias_h + 8 * 256, Xh, Xl, Xh, Xl, Yh, Yl, true);    // L7 -> Y = relu(h7); requests the feature layer's first bias
    sig = gemmx_tile<16, 0, 0, true>(r, Yh, Yl, Yh, Yl);                                       // sigma head (ahead of the feature layer)
    if constexpr (DSKIP) {
      // in front of the wave-uniform branch everything in flight lands (the three pairs the sigma head prefetched past its end, the
      // feature layer's first bias quad): the compiler copies registers on the edges into the two arms (one exposed LDS round
      // trip per 128-point tile)
      xring_drain_reads(r, nb);
      dead_wave = __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(
                      h == 0 && valid && sig[0] + hb_s > 0.0f) != 0ull)) == 0;
    }
    if constexpr (DENS) {
      // density only (coarse pass of a hierarchical render, volume_renderer.py:335): the stream wraps after the sigma chunk,
      // which the head's 16 steps consume exactly, so the ring advances by itself
#pragma unroll
      for (int i = 0; i < 16; ++i) col[i] = 0.0f;
    } else if (dead_wave) {
      // no density in this wave's 32 points: the colour branch's chunks go by unread (what the sigma head prefetched past its
      // end has landed above and is simply dropped)
#pragma unroll 1
      for (int c = 0; c < kColourChunks; ++c) {
#pragma unroll
        for (int i = 0; i < kXDmaPerWave; ++i) xring_issue_part(r, i);
        xring_advance(r);
      }
      xring_prime_sync(r);              // (landed before the branches join: the compiler copies registers there)
#pragma unroll
      for (int i = 0; i < 16; ++i) col[i] = 0.0f;
    } else {
      gemmx_layer<16, 0, 8, 0, true>(r, nb, bias_h + 8 * 256, bias_views_h, Yh, Yl, Yh, Yl, Xh, Xl, false);       // feature
      h8 Vh[8], Vl[8];
      gemmx_layer<16, 2, 4, 0, false>(r, nb, bias_views_h, bias_views_h, Xh, Xl, DPEh, DPEl, Vh, Vl, true);      // views
      col = gemmx_tile<8, 0, 8, true>(r, Vh, Vl, Vh, Vl);                                        // rgb head
    }
    // end of the tile on every path: request the bias of the next tile's (L0, out-tile 0) and let EVERYTHING in flight land -- the
    // pairs prefetched for the next tile's first steps stay valid in their registers, and no asm read is in flight across the
    // join of the branches or the loop's back edge (one exposed LDS round trip per 128-point tile)
    xbias_read_asm(bias_h, nb);
    xring_drain_reads(r, nb);
    }

    if (valid && h == 0) {
      f32x4 out;
      const bool no_colour = DENS || dead_wave;
      out.x = no_colour ? 0.0f : col[0] + hb_r;
      out.y = no_colour ? 0.0f : col[1] + hb_g;
      out.z = no_colour ? 0.0f : col[2] + hb_b;
      out.w = sig[0] + hb_s;
      reinterpret_cast<f32x4*>(a.raw)[p] = out;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
