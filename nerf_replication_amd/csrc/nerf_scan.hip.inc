// Ordered lists without atomics: the rank of a thread inside its 256-thread block, and the one-workgroup scan that turns the
// block totals into offsets.  Used by the live-tile list (nerf_train_backward.hip.inc), the ordered compaction
// (nerf_sampling.hip.inc), the iso-surface (nerf_isosurface.hip.inc) and the mesh clean-up (nerf_mesh_components.hip.inc).
#pragma once

namespace {

// ------------------------------------------------------------------------------------ rank inside a block
constexpr int kRankBlock = 256;

// Every wave brings its total (read from lane `writer_lane`): the sum over the waves in front of this one, block_total = all
__device__ __forceinline__ int block_waves_before(int wave_total, int writer_lane, int* s_wave, int& block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == writer_lane) s_wave[wave] = wave_total;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kRankBlock / 64; ++w) {
    const int c = s_wave[w];
    if (w < wave) before += c;
    total += c;
  }
  block_total = total;
  return before;
}
// number of threads in front of this one with `v` set
__device__ __forceinline__ int compact_block_rank(bool v, int* s_wave, int& block_total) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(v);
  const int lane = threadIdx.x & 63;
  return block_waves_before((int)__popcll(m), 0, s_wave, block_total) + (int)__popcll(m & ((1ull << lane) - 1ull));
}
// sum of `v` over the threads in front of this one (v < 2^16 per thread; two 16-bit fields are scanned as one int by the caller)
__device__ __forceinline__ int iso_block_exclusive(int v, int* s_wave, int& block_total) {
  const int lane = threadIdx.x & 63;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  return block_waves_before(inc, 63, s_wave, block_total) + inc - v;
}

// ------------------------------------------------------------------------------------ scan by one workgroup
// Exclusive scan over value(0) .. value(n - 1) by ONE workgroup of kScanThreads threads (the lists are a few thousand entries):
// thread t sums its chunk of ceil(n / 1024) consecutive items, a Hillis-Steele pass over the 1024 partial sums in `s_sum`, then
// emit(i, sum of the values in front of i) for its chunk in order.  A thread whose chunk would start past the end has the empty
// chunk [n, n).  value(i) is read before emit(i, .) is called, so emit may overwrite what value reads.  Returns the total (in
// every thread).  T: zero-initialised by T{}, with + and -.
constexpr int kScanThreads = 1024;
template <class T, class Value, class Emit>
__device__ __forceinline__ T workgroup_scan(long long n, T* s_sum, Value value, Emit emit) {
  const int tid = threadIdx.x;
  const long long per = (n + kScanThreads - 1) / kScanThreads;
  const long long i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
  T own{};
  for (long long i = i0; i < i1; ++i) own = own + value(i);
  s_sum[tid] = own;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const T v = tid >= d ? s_sum[tid - d] : T{};
    __syncthreads();
    s_sum[tid] = s_sum[tid] + v;
    __syncthreads();
  }
  T run = s_sum[tid] - own;
  for (long long i = i0; i < i1; ++i) {
    const T v = value(i);
    emit(i, run);
    run = run + v;
  }
  return s_sum[kScanThreads - 1];
}

}  // namespace
