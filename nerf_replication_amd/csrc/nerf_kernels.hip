// libnerf_mi355x.so, first translation unit -- HIP kernels (gfx950 only) and the C ABI of include/nerf_mi355x.h.
// Build: hipcc -O3 --offload-arch=gfx950 -shared -fPIC (see csrc/Makefile).  This file is the unit's table of contents: every kernel
// and every entry lives in the file named here, in an order in which each finds what it needs ahead of it.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <utility>

#include "../../include/nerf_mi355x.h"
#include "nerf_host.h"                 // fail / launch / NERF_LAUNCH, num_cus, align256, Carver
#include "nerf_mlp_common.h"           // types, MlpArgs / BwdArgs, TrainSave / TrainGrad, shared device helpers (+ nerf_layout.h)
#include "nerf_wgrad_table.h"
#include "nerf_scan.hip.inc"
// ---- the MLP and weight-gradient kernels
#include "nerf_mlp_f32.hip.inc"
#include "nerf_mlp_f16.hip.inc"
#include "nerf_mlp_f16s.hip.inc"
#include "nerf_mlp_f32x.hip.inc"
#include "nerf_wgrad_f32.hip.inc"
#include "nerf_mlp_bwd_f32.hip.inc"
#include "nerf_mlp_bwd_f32x.hip.inc"
#include "nerf_wgrad_bf16x3.hip.inc"
// the split-fp16 MLP kernels are compiled in a unit of their own (nerf_kernels_x.hip says why); here they are only launched
#define NERF_X_INST extern template
#include "nerf_kernels_x.inst.inc"

#include "nerf_timing_guard.h"         // after the kernel includes: refuses a build with a stray timing switch

// ---- the core: kernels and entries, one file per subsystem
#include "nerf_pack.hip.inc"             // nerf_pack_model[_bwd], nerf_pack_model_ordered, nerf_packed_*_bytes
#include "nerf_unit_order.hip.inc"       // nerf_unit_order_stats / _match (include/nerf_mi355x_order.h)
#include "nerf_sampling.hip.inc"         // nerf_sample_fine*, nerf_stratified_samples, nerf_compact_valid
#include "nerf_composite.hip.inc"        // nerf_composite[_backward]
#include "nerf_mlp_launch.hip.inc"       // nerf_mlp_forward*: inference and SAVE
#include "nerf_train_backward.hip.inc"   // nerf_mlp_backward*, nerf_wgrad, the ray adjoints, nerf_adam_step
#include "nerf_image.hip.inc"            // nerf_generate_rays, nerf_positional_encoding, nerf_image_metrics / _ssim
#include "nerf_frame.hip.inc"            // nerf_render_forward[_stochastic]
// ---- geometry out of a trained network: nerf_isosurface_* (kernels and entries)
#include "nerf_isosurface.hip.inc"
// ---- occupancy grid: nerf_occupancy_* and nerf_render_forward_occupancy
#include "nerf_occupancy.hip.inc"
// ---- geometry outputs: nerf_density_gradient and nerf_composite_normals
#include "nerf_normals.hip.inc"
// ---- mesh clean-up: nerf_mesh_components and nerf_mesh_filter_*
#include "nerf_mesh_components.hip.inc"
// ---- multiresolution hash-grid encoding: nerf_hashgrid_forward / nerf_hashgrid_backward
#include "nerf_hashgrid.hip.inc"
// ---- its deterministic table gradient (include/nerf_mi355x_hashgrid.h): nerf_hashgrid_backward_deterministic
#include "nerf_hashgrid_det.hip.inc"
// ---- small fused ReLU MLP (include/nerf_mi355x_nn.h): nerf_fused_mlp_forward / nerf_fused_mlp_backward
#include "nerf_fused_mlp.hip.inc"
// ---- its exact weight and bias gradients (include/nerf_mi355x_nn_exact.h): nerf_fused_mlp_backward_exact
#include "nerf_fused_mlp_exact.hip.inc"
// ---- hash-grid radiance field, the ray-side glue (include/nerf_mi355x_nn.h): nerf_sh4_encode, nerf_field_*
#include "nerf_hashfield.hip.inc"
// ---- where its samples lie (include/nerf_mi355x_sampling.h): nerf_field_sample_importance, nerf_field_stratified_depths
#include "nerf_field_sampling.hip.inc"
// ---- the deformation field of a dynamic scene (include/nerf_mi355x_deform.h): nerf_deform_forward / _backward / _pack / _unpack_grad
#include "nerf_deform.hip.inc"

extern "C" {

int32_t nerf_abi_version(void) { return NERF_ABI_VERSION; }

int32_t nerf_build_flags(void) {
  int32_t f = 0;
#ifdef NERF_TIMING_BUILD
  f |= NERF_BUILD_TIMING;
#endif
#if NERF_ANY_TIMING_HACK || NERF_SAVE_TAPS == 0
  f |= NERF_BUILD_WRONG_NUMERICS;
#endif
  return f;
}
const char* nerf_last_error(void) { return g_err; }

}  // extern "C"
