// Recorder of tests/golden/wgrad_choice.txt: which fp32 weight-gradient instance, with which wave split, wgrad_impl chose
// for a layer shape BEFORE the choice became a table (csrc/nerf_wgrad_table.h).  The two macro chains below are that
// wgrad_impl's, verbatim, with every launch reduced to "which instance, which split"; the batched 256 x 256 ring launch ahead
// of them depends on the point count and is not part of the choice.  tests/test_wgrad_choice.py holds the table to this record.
//
//     c++ -std=c++17 -o record_wgrad_choice tools/record_wgrad_choice.cpp && ./record_wgrad_choice > tests/golden/wgrad_choice.txt
//
// One line per shape and combination of facts: n_out n_in facts instance osplit isplit, facts = aligned + 2 hin8 + 4 ring + 8 live.
// Instances: f32<TO,TI> = nerf_wgrad_f32_kernel<TO,TI>; vec<AV,BV> = nerf_wgrad_vec_f32_kernel<AV,BV>; ring<AV,BV,16> and
// list<AV,BV,16> = nerf_wgrad_vec_f32_asm_kernel<AV,BV,16> without and with LIST; w256 = nerf_wgrad256_f32_kernel; none = the
// error "live-tile list on a shape without an asm-ring kernel".
#include <cstdio>

static void chosen(int n_out, int n_in, int facts, const char* instance, int osplit, int isplit) {
  std::printf("%d %d %d %s %d %d\n", n_out, n_in, facts, instance, osplit, isplit);
}

static void choose(int n_out, int n_in, int facts) {
  const bool aligned = facts & 1, hin8 = facts & 2, ring = facts & 4, live = facts & 8;
  const int to = (n_out + 31) / 32, ti = (n_in + 31) / 32;
#define RETURN(NAME, OS, IS) do { chosen(n_out, n_in, facts, NAME, OS, IS); return; } while (0)
  if (live && !ring) RETURN("none", 0, 0);
  if (!live && n_out == 256 && n_in == 256 && aligned) RETURN("w256", 2, 2);
#define VEC(AV, BV, OS, IS) do { \
    if (live) RETURN("list<" #AV "," #BV ",16>", OS, IS); \
    if (ring) RETURN("ring<" #AV "," #BV ",16>", OS, IS); \
    RETURN("vec<" #AV "," #BV ">", OS, IS); \
  } while (0)
  if (n_out == 256 && n_in <= 64 && aligned) VEC(4, 1, 2, 2);                  // PE -> 256 (layers 0 and 5)
  if (n_out == 128 && n_in == 256 && aligned) VEC(4, 2, 1, 4);                 // views_linears.0, feature part
  if (n_out == 128 && n_in <= 32) VEC(1, 1, 4, 1);                             // views_linears.0, direction part
  if (n_out <= 32 && n_in == 256 && hin8) VEC(1, 2, 1, 4);                     // alpha_linear
  if (n_out <= 32 && n_in <= 128) VEC(1, 1, 1, 4);                             // rgb_linear
#undef VEC
  if (live) RETURN("none", 0, 0);
#define GEN(TO, TI, OS, IS) RETURN("f32<" #TO "," #TI ">", OS, IS)
  if (to > 4 && ti > 2) GEN(4, 4, 2, 2);
  if (to > 4) GEN(4, 1, 2, 2);
  if (to > 1 && ti > 4) GEN(2, 4, 2, 2);
  if (to > 2 && ti > 1) GEN(2, 2, 2, 2);
  if (to > 1 && ti > 2) GEN(1, 2, 2, 2);
  if (to > 1 && ti > 1) GEN(1, 1, 2, 2);
  if (to > 1) GEN(1, 1, 4, 1);
  if (ti > 4) GEN(1, 2, 1, 4);
  GEN(1, 1, 1, 4);
#undef GEN
#undef RETURN
}

int main() {
  const int sizes[] = {1, 3, 27, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256};
  for (int n_out : sizes)
    for (int n_in : sizes)
      for (int facts = 0; facts < 16; ++facts) choose(n_out, n_in, facts);
  return 0;
}
