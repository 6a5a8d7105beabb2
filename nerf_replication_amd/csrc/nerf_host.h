// Host side of every entry of the C ABI: the error text behind nerf_last_error(), the checked kernel launch, the device's CU
// count and the workspace carver.  Host only: included by nerf_kernels.hip and by every file with entries (csrc/nerf_*.hip.inc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/nerf_mi355x.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* what) {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return code;
}
// Every kernel launch: NERF_OK, or NERF_ERR_HIP with "<kernel>: <hip error>" in nerf_last_error().  NERF_LAUNCH names the kernel
// expression as it is written at the call (a template instance with a comma in its arguments is written, and reported, in
// parentheses).
template <class K, class... Args>
int launch(const char* name, K kernel, dim3 grid, dim3 block, hipStream_t st, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return NERF_OK;
  snprintf(g_err, sizeof(g_err), "%s: %s", name, hipGetErrorString(e));
  return NERF_ERR_HIP;
}
#define NERF_LAUNCH(kernel, grid, block, stream, ...) launch(#kernel, kernel, grid, block, stream, __VA_ARGS__)

// ------------------------------------------------------------------------------------ launch helpers
int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    cus = v;
  }
  return cus;
}

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Every workspace is ONE layout struct that takes its pieces from a Carver, in order, each 256-byte aligned: built on the
// caller's pointer it holds the pieces, built on a null base its bytes() is what the *_workspace_bytes entry reports.
struct Carver {
  uintptr_t base, p;
  explicit Carver(const void* b) : base((uintptr_t)b), p((uintptr_t)b) {}
  template <class T> T* take(int64_t count) {
    T* q = (T*)p;
    p += (uintptr_t)align256(count * (int64_t)sizeof(T));
    return q;
  }
  int64_t bytes() const { return (int64_t)(p - base); }
};

}  // namespace
