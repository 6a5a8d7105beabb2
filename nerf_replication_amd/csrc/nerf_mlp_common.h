// What the MLP kernel files (csrc/nerf_mlp_*.hip.inc), the files that launch them and both translation units share: the vector and
// address-space types, the argument structs of the forward and the backward chain with the layouts of their save buffers, the
// small device helpers, and the workgroup / LDS-ring constants that more than one file reads.  Device and host.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

#include "nerf_layout.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

// LDS (address space 3) and global (1) pointees: the LDS-DMA builtin and the ds_read paths want the address space in the type
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef const __attribute__((address_space(3))) float lds_cfloat;
typedef const __attribute__((address_space(3))) f32x2 lds_cf32x2;
typedef const __attribute__((address_space(3))) f32x4 lds_cf32x4;
typedef const __attribute__((address_space(3))) h8 lds_ch8;

// Workgroup shapes and the LDS ring of the fp16-operand kernels (f16, f16s: 8 waves; f32x and its backward chain: 4 waves, one
// per SIMD): read by the kernels and by the host that launches them
constexpr int kF16Waves = 8;
constexpr int kF16Threads = kF16Waves * 64;
constexpr int kF16TilePts = kF16Waves * 32;                 // points per workgroup tile
constexpr int kF16RingSlots = 4;
constexpr int kF16LdsBytes = nerf::kF16ConstBytes + kF16RingSlots * nerf::kF16ChunkBytes;   // 147456
constexpr int kXWaves = 4;
constexpr int kXThreads = kXWaves * 64;
constexpr int kXTilePts = kXWaves * 32;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Branch-free sin/cos for |x| < ~1e4: 3-term Cody-Waite reduction by pi/2 (FMA) + the classic
// single-precision minimax polynomials on [-pi/4, pi/4]; abs error ~1e-7.  Small register
// footprint and no slow path, so it can sit in the middle of the kernel (the ocml sincosf's
// large-argument path forced ~50 spills when placed between layers).
__device__ __forceinline__ void sincos_cw(float x, float& s, float& c) {
  const float n = rintf(x * 0.636619772367581343f);            // x * 2/pi
  float r = fmaf(n, -1.5703125f, x);
  r = fmaf(n, -4.837512969970703125e-4f, r);
  r = fmaf(n, -7.54978995489188216e-8f, r);
  const float r2 = r * r;
  const float sp = fmaf(r * r2, fmaf(r2, fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), r);
  const float cp = fmaf(r2 * r2, fmaf(r2, fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                        fmaf(r2, -0.5f, 1.0f));
  const int q = (int)n;
  const float ss = (q & 1) ? cp : sp;
  const float cc = (q & 1) ? sp : cp;
  s = (q & 2) ? -ss : ss;
  c = ((q + 1) & 2) ? -cc : cc;
}

// Wave-uniform load of a word that no kernel of the same launch writes (live-tile list, its count), through the CONSTANT address
// space: hipcc then emits s_load_dword.  As a plain global load it becomes a vector load + v_readfirstlane (it cannot prove the
// list invariant next to the kernels' own stores and atomics) whose result it waits for with vmcnt(0) -- which, once per step of
// a list-mode weight-gradient kernel, drained the whole LDS-DMA / asm-load pipeline (round 3, LAB_NOTEBOOK.md A11).
__device__ __forceinline__ int uniform_load_i32(const int* p) {
  return *(const __attribute__((address_space(4))) int*)p;
}

template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

struct MlpArgs {
  const float* pts;        // [P,3] explicit points, or nullptr -> o + d*t
  const float* rays_o;     // [N,3]
  const float* rays_d;     // [N,3]
  const float* viewdirs;   // [N,3] or nullptr -> rays_d / ||rays_d||
  const float* tvals;      // t of (ray, s) at tvals[ray*t_ray_stride + s]
  long long t_ray_stride;  // 0: all rays share one t table
  long long n_points;      // P = N*S
  int n_samples;           // S
  int tile_rays_log2;      // fp32 inference ray instances without a list: a tile is (1 << lg) neighbouring rays by (32 >> lg) consecutive
                           // samples instead of 32 consecutive samples of one ray (0) -- shorter along the ray, so more k-steps are dead
                           // tile-wide; raw is bit-identical.  forward_rays: 0 unless (32 >> lg) divides n_samples.
                           // Sits in what was padding behind n_samples: no other field moves and no other kernel's ISA changes
  const float* packed;     // nerf_layout.h packed model
  float* raw;              // [P,4] = (r,g,b,sigma) pre-activation
  const int* index;        // optional (ray mode): compacted list of point ids to evaluate (masked fine pass)
  const int* count;        // device count of entries in `index`
  float* save;             // SAVE mode (training forward): activation store, see TrainSave
  int skip_dead_colour;    // ray mode, fp32 inference kernel: tiles without a single sigma > 0 stop after the sigma head (DSKIP)
  int density_only;        // ray mode, fp32 kernel: stop after the sigma head (raw = (0,0,0,sigma)): the coarse pass of a
                           // hierarchical render / training step, whose colour is never read (volume_renderer.py:335 / SURVEY F6)
  const float* fold;       // fp32 kernels: packed + kOffFold, the fold region of `packed` (nerf_layout.h kFold*), written by
                           // nerf_pack_model (launch_mlp)
  int skip_dead_ksteps;    // fp32 inference instances: a k-step whose ReLU-output activation register is zero in all 64 lanes
                           // issues no MFMAs (gemm_tiles KSKIP; bit-identical raw).  launch_mlp: 1 unless NERF_DEAD_KSTEP_SKIP=0
  int skip_dead_groups;    // with skip_dead_ksteps: the leading run of all-dead 4-k-step groups of such a GEMM costs no wait, no
                           // loads and no row branches (gemm_tiles `prefix`).  launch_mlp: 1 unless NERF_DEAD_GROUP_SKIP=0
};

// Training forward keeps what the backward pass needs, row-major per point (the layout the weight-
// gradient GEMMs read coalesced): P = n_points, offsets in floats.
struct TrainSave {
  static constexpr int kPe = 64, kDpe = 32;        // xyz / dir encodings in REFERENCE channel order, zero padded
  // Every region holds pad32(P) rows: the fp32 kernels let the idle lanes of a ragged last tile store their
  // (duplicate) rows into the padding instead of predicating ~300 stores per tile.
  static constexpr long long pad32(long long P) { return (P + 31) & ~31LL; }
  static constexpr long long off_pe(long long P) { return 0; }
  static constexpr long long off_dpe(long long P) { return pad32(P) * 64; }
  static constexpr long long off_h(long long P, int l) { return pad32(P) * (96 + 256LL * l); }      // h0..h7 (post-ReLU)
  static constexpr long long off_f(long long P) { return pad32(P) * (96 + 2048); }                  // feature (no ReLU)
  static constexpr long long off_hv(long long P) { return pad32(P) * (96 + 2304); }                 // views (post-ReLU) [P,128]
  // ReLU sign bits for the fp32 backward chain: per 32-point tile and masked tensor (0..7 = h0..h7, 8 = views) one
  // 1-KiB block = 64 lanes x 4 dwords in ACCUMULATOR layout (lane (p,h), bit 16*t + r of its 128 bits <-> feature
  // act_feat(t, r, h) > 0): the backward kernel fetches a layer's mask with ONE coalesced 16-byte load per lane instead
  // of re-reading the 1-KiB activation row of every point.  Written by the fp32 SAVE forward only.
  static constexpr int kMasked = 9;
  static constexpr long long off_bits(long long P) { return pad32(P) * (96 + 2304 + 128); }
  static constexpr long long bits_block(long long tile, int which) { return ((tile * kMasked + which) * 64) * 4; }   // floats
  // one word (+ padding) behind everything: what the forward that filled the buffer did with density-free tiles
  // (0 = every row stored, != 0 = their h7 / feature / views rows and colour-branch bits are absent): dead_tile_list_available
  static constexpr long long off_stamp(long long P) { return off_bits(P) + (pad32(P) / 32) * kMasked * 256; }
  static constexpr long long floats(long long P) { return off_stamp(P) + 4; }
};

struct BwdArgs {
  const float* rays_o; const float* rays_d; const float* tvals; long long t_ray_stride;
  long long n_points; int n_samples;
  const float* packed_bwd;   // transposed stream + head weights (nerf_layout.h kBwd*)
  const float* draw;         // [P,4] gradient of raw (r,g,b,sigma)
  const float* save;         // TrainSave of the forward
  float* gsave;              // TrainGrad: g_zv [P,128], g_f [P,256], g_z7..g_z0 [P,256] each
  float* g_t;                // optional [P]: d loss / d t through the points (= g_x . rays_d).  Ray mode, bit 0 set: the address
                             // (bit cleared) of g_x [P,3] = d loss / d (o + d t) instead, written in place of g_t (the launcher's
                             // encoding, mlp_backward_impl: ONE output pointer stays live across the chain, as before; a second
                             // one cost the f32x density chain an SGPR spill to scratch)
  // point mode (Network.forward under autograd, network.py:199-258: explicit points instead of o + d*t)
  const float* pts;          // [P,3]
  float* g_x;                // optional [P,3]: d loss / d points
  int density_only;          // fp32 chain: d loss / d rgb is identically zero (coarse pass of a training step): the colour
                             // branch (views, feature) is skipped, the chain starts at g_h7 = w_alpha * g_sigma
  // live-tile list (fp32 chain, optional): workgroup slot i handles the 32-point tile live_tiles[i], slots >= *n_live exit.
  // A tile is dead when d loss / d raw is zero at all of its points -- then every g_z of the tile is zero, so are its
  // contributions to the weight gradients and to g_t / g_x, and nothing of it needs computing (see nerf_tile_flags_kernel)
  const int* live_tiles;
  const int* n_live;
};

struct TrainGrad {          // pad32(P) rows per region, like TrainSave
  static constexpr long long off_gzv(long long P) { return 0; }
  static constexpr long long off_gf(long long P) { return TrainSave::pad32(P) * 128; }
  static constexpr long long off_gz(long long P, int l) { return TrainSave::pad32(P) * (384 + 256LL * (7 - l)); }   // l = 7..0
  // behind the rows, as 32-bit integers: one flag per 32-point tile, the ascending list of live tiles, their count
  static constexpr long long n_tiles(long long P) { return TrainSave::pad32(P) / 32; }
  static constexpr long long off_flags(long long P) { return TrainSave::pad32(P) * (384 + 2048); }
  static constexpr long long off_live(long long P) { return off_flags(P) + ((n_tiles(P) + 3) & ~3LL); }
  static constexpr long long off_count(long long P) { return off_live(P) + ((n_tiles(P) + 3) & ~3LL); }
  static constexpr long long floats(long long P) { return off_count(P) + 4; }
};
