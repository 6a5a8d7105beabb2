// Which fp32 weight-gradient kernel serves a layer shape: one ordered table and one pure function, no HIP in it (a host
// compiler alone builds it: tests/test_wgrad_choice.py).  nerf_train_backward.hip.inc instantiates the kernels from the same rows.
//
// Every kernel gives each of its 4 waves `wo` x `wi` 32x32 output tiles and splits the waves osplit x isplit, so a row
// covers 32*wo*osplit outputs and 32*wi*isplit inputs.  A row that does not cover the shape is never eligible; the first
// eligible row is taken.  (The batched 256 x 256 ring launch is tried ahead of the table: its conditions are on the
// point count, not on the shape.)
#pragma once

namespace nerf {

enum WgKind {
  kWgGeneric,      // nerf_wgrad_f32_kernel<wo, wi>: scalar loads, tile-contiguous columns, any alignment
  kWgVec,          // nerf_wgrad_vec_f32_kernel<wo, wi>: one wo- / wi-float load per lane and row, interleaved columns
  kWgVecRing       // the same, and nerf_wgrad_vec_f32_asm_kernel<wo, wi, 16> (whole point range or live-tile list) when `ring`
};
enum WgAlign { kWgAnyAlign, kWgHin8, kWgAligned16 };
enum WgForm { kWgPlain, kWgRing, kWgList, kWgNoListKernel };    // the last: a live-tile list on a shape without an asm-ring kernel

struct WgRow {
  WgKind kind;
  int wo, wi;                  // tiles (= floats per lane and row, for the vector-load kernels) per wave: out, in
  int osplit, isplit;          // osplit * isplit == 4 waves
  WgAlign align;               // what the operands must be aligned to
  bool exact_out, exact_in;    // the row serves only shapes that fill it on this side (its lanes load whole vectors)
  constexpr int outs() const { return 32 * wo * osplit; }
  constexpr int ins() const { return 32 * wi * isplit; }
};

constexpr WgRow kWgRows[] = {
    {kWgVec, 4, 4, 2, 2, kWgAligned16, true, true},          // the 256 x 256 layers, off the batched ring launch
    {kWgVecRing, 4, 1, 2, 2, kWgAligned16, true, false},     // PE -> 256 (layers 0 and 5)
    {kWgVecRing, 4, 2, 1, 4, kWgAligned16, true, true},      // views_linears.0, feature part
    {kWgVecRing, 1, 1, 4, 1, kWgAnyAlign, true, false},      // views_linears.0, direction part
    {kWgVecRing, 1, 2, 1, 4, kWgHin8, false, true},          // alpha_linear
    {kWgVecRing, 1, 1, 1, 4, kWgAnyAlign, false, false},     // rgb_linear
    // everything else, smallest cover first (the rows of 2..4 input tiles serve the square and near-square layers of
    // nerf_fused_mlp_backward, 64 x 64 and 128 x 128, which the lego network does not have; up to 32 x 128 is the rgb_linear row's)
    {kWgGeneric, 1, 2, 1, 4, kWgAnyAlign, false, false},
    {kWgGeneric, 1, 1, 4, 1, kWgAnyAlign, false, false},
    {kWgGeneric, 1, 1, 2, 2, kWgAnyAlign, false, false},
    {kWgGeneric, 1, 2, 2, 2, kWgAnyAlign, false, false},
    {kWgGeneric, 2, 2, 2, 2, kWgAnyAlign, false, false},
    {kWgGeneric, 2, 4, 2, 2, kWgAnyAlign, false, false},
    {kWgGeneric, 4, 1, 2, 2, kWgAnyAlign, false, false},
    {kWgGeneric, 4, 4, 2, 2, kWgAnyAlign, false, false},
};
constexpr int kWgNumRows = sizeof(kWgRows) / sizeof(kWgRows[0]);

struct WgFacts {
  bool aligned;    // both operands: 16-byte base, leading dimension and first column multiples of 4 floats
  bool hin8;       // hin alone: 8-byte base, leading dimension and first column multiples of 2 floats
  bool ring;       // whole groups of 32 points and 32-bit byte strides: the host contract of the asm-ring kernels
  bool live;       // the point range is a live-tile list
};
struct WgChoice { int row; WgForm form; };

constexpr bool wg_eligible(const WgRow& r, int n_out, int n_in, const WgFacts& f) {
  return (r.exact_out ? n_out == r.outs() : n_out <= r.outs()) && (r.exact_in ? n_in == r.ins() : n_in <= r.ins()) &&
         (r.align == kWgAnyAlign || (r.align == kWgHin8 && f.hin8) || (r.align == kWgAligned16 && f.aligned));
}

// 1 <= n_out, n_in <= 256.  A list needs a ring row and the ring contract; nothing else may serve it.
constexpr WgChoice wg_choose(int n_out, int n_in, const WgFacts& f) {
  for (int i = 0; i < kWgNumRows; ++i)
    if (wg_eligible(kWgRows[i], n_out, n_in, f)) {
      const bool ring = kWgRows[i].kind == kWgVecRing && f.ring;
      return {i, f.live ? (ring ? kWgList : kWgNoListKernel) : (ring ? kWgRing : kWgPlain)};
    }
  return {-1, kWgNoListKernel};
}

constexpr bool wg_rows_sound() {
  for (int i = 0; i < kWgNumRows; ++i)
    if (kWgRows[i].osplit * kWgRows[i].isplit != 4) return false;
  // every shape the entry accepts, by tile count, at both ends of each tile and with no fact in its favour
  for (int to = 1; to <= 8; ++to)
    for (int ti = 1; ti <= 8; ++ti)
      for (int lo = 0; lo < 4; ++lo) {
        const int n_out = 32 * to - 31 * (lo & 1), n_in = 32 * ti - 31 * (lo >> 1);
        const WgChoice c = wg_choose(n_out, n_in, WgFacts{false, false, false, false});
        if (c.row < 0 || kWgRows[c.row].outs() < n_out || kWgRows[c.row].ins() < n_in) return false;
      }
  return true;
}
static_assert(wg_rows_sound(), "some row must cover every shape up to 256 x 256, whatever its alignment");

}  // namespace nerf
