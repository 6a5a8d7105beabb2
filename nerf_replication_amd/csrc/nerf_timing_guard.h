// Included by every translation unit of libnerf_mi355x.so AFTER its kernel includes (which give the switches their defaults).
// Timing-only switches (tools/ab_bench.py) change the NUMERICS of the kernels they are compiled into.  A library
// built with any of them set must say so: it only compiles with -DNERF_TIMING_BUILD, and then reports it through
// nerf_build_flags(), which the Python loader (and any other binder) checks -- so a stray -D can no longer produce a
// library that passes nerf_abi_version() and computes garbage, whichever unit the switch acts in.  (A unit that does not
// include the file that owns a switch sees the name undefined: 0 in #if, unless the command line set it.)
#pragma once
#define NERF_ANY_TIMING_HACK (NERF_F32_HACK_NOBIAS || NERF_F32_ASM_OVERRUN || NERF_F32_HACK_NOSAVE || NERF_BWD_HACK_NOMASK || \
                              NERF_F16_HACK_NOADV || NERF_F16_HACK_NOBARRIER || NERF_WG_HACK_NOATOMIC || NERF_F16_HACK_NOEPI || \
                              NERF_F16_HACK_NORELU || NERF_F32X_HACK_NOADV || NERF_F32X_HACK_NOPE || NERF_F32X_HACK_NOEPI || \
                              NERF_F32X_HACK_SAVE_NOSTORE || NERF_XB_HACK_NOSTORE)
// (a structural knob of the SAVE forward also breaks results when switched off: no rows stored.  Its default is 1, so in a unit
// without nerf_mlp_f32.hip.inc, which owns it, the name counts only where the command line set it)
#if (NERF_ANY_TIMING_HACK || (defined(NERF_SAVE_TAPS) && NERF_SAVE_TAPS == 0)) && !defined(NERF_TIMING_BUILD)
#error "a NERF_*_HACK_* / NERF_F32_ASM_OVERRUN timing switch is set: such a library computes wrong results; build it with -DNERF_TIMING_BUILD (tools/ab_bench.py does) so that nerf_build_flags() reports it"
#endif
