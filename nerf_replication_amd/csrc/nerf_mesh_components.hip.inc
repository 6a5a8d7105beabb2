// Connected components of an indexed triangle mesh and the filter that keeps whole components (DESIGN.md section 2.11).
// Needs nerf_sampling.hip.inc ahead of it (the ordered compaction's nerf_compact_scan_kernel); compact_block_rank comes from
// nerf_scan.hip.inc.
//
// Union-find over parent[V] (int32), lock-free.  A root is always linked under a SMALLER root, so parent[x] <= x holds at every
// moment, every chain strictly descends, and the root a tree ends up with is the smallest id in it whatever the order in which the
// faces arrive: the labels are unique, and two runs write the same bytes although the links are made with atomics.
//
// What the loops rely on, and what they do not:
//   * parent[x] is only ever overwritten with an id further down x's own chain (a link x -> smaller root by the one successful
//     atomicCAS that ends x's time as a root; later the path-splitting atomicMin, which only lowers it).  Every value parent[x] has
//     ever held is therefore <= x and in x's component, so a STALE value (another XCD's L2, a CU's L1) is still a correct, merely
//     longer, way down: mc_find ends after at most x steps on any mixture of old and new values.  The loads are agent-scope relaxed
//     atomics all the same (they bypass the L1).
//   * whether x is still a root is decided by the atomicCAS alone, never by re-reading.  A failed CAS returns the id x was linked
//     under (< x) and the union goes on from there: a + b strictly falls with every failed CAS.  No loop waits for another thread.
//   * labels are read only in later launches than the unions (the kernel boundary is the synchronisation).

#include "nerf_host.h"
#include "nerf_scan.hip.inc"

namespace {

constexpr int kMcBlock = kRankBlock;         // compact_block_rank's block

__device__ __forceinline__ int mc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the lowest id reachable from x; path splitting on the way (every visited node is re-pointed at its grandparent)
__device__ __forceinline__ int mc_find(int* parent, int x) {
  int p = mc_load(parent + x);
  while (p < x) {                               // p == x: a root.  (p > x cannot happen; it would end the walk as well)
    const int gp = mc_load(parent + p);
    if (gp < p) atomicMin(parent + x, gp);      // x is no root (p < x) and stays none: the CAS below never sees this store
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void mc_union(int* parent, int a, int b) {
  a = mc_find(parent, a);
  b = mc_find(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }          // a: the larger of the two
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;                                  // a was a root and now hangs under b < a
    a = mc_find(parent, old);                              // a had been linked already, under old < a: go on from there
    b = mc_find(parent, b);
  }
}

__device__ __forceinline__ bool mc_face_ok(int v0, int v1, int v2, int V) {
  return (unsigned)v0 < (unsigned)V && (unsigned)v1 < (unsigned)V && (unsigned)v2 < (unsigned)V;
}

__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_init_kernel(int V, int* __restrict__ parent, int* __restrict__ cnt_f, int* __restrict__ cnt_v) {
  const long long v = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  if (v < V) { parent[v] = (int)v; cnt_f[v] = 0; cnt_v[v] = 0; }
}

__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_union_kernel(const int* __restrict__ faces, int T, int V, int* __restrict__ parent) {
  const long long t = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  if (t >= T) return;
  const int v0 = faces[3 * t], v1 = faces[3 * t + 1], v2 = faces[3 * t + 2];
  if (!mc_face_ok(v0, v1, v2, V)) return;                   // joins nothing; no index of it is read through
  if (v1 != v0) mc_union(parent, v0, v1);
  if (v2 != v0 && v2 != v1) mc_union(parent, v0, v2);
}

// a launch of its own behind the unions: every root is final, label[v] = the root of v
__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_flatten_kernel(int V, int* __restrict__ parent, int* __restrict__ vertex_label) {
  const long long v = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  if (v < V) vertex_label[v] = mc_find(parent, (int)v);
}

// counts[label] += 1 for every thread with label >= 0; the lanes that share lane 0's label add once for all of them
__device__ __forceinline__ void mc_count(int* __restrict__ counts, int label) {
  const int first = __builtin_amdgcn_readfirstlane(label);
  const bool same = label == first;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(same);
  if (label < 0) return;
  if (!same) atomicAdd(counts + label, 1);
  else if ((threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counts + label, (int)__popcll(m));
}

// thread i: face i's label and its component's face count, vertex i's component's vertex count
__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_count_kernel(const int* __restrict__ faces, int T, int V, const int* __restrict__ vertex_label,
                            int* __restrict__ face_label, int* __restrict__ cnt_f, int* __restrict__ cnt_v) {
  const long long i = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  int fl = -1;
  if (i < T) {
    const int v0 = faces[3 * i], v1 = faces[3 * i + 1], v2 = faces[3 * i + 2];
    if (mc_face_ok(v0, v1, v2, V)) fl = vertex_label[v0];
    face_label[i] = fl;
  }
  mc_count(cnt_f, fl);
  mc_count(cnt_v, i < V ? vertex_label[i] : -1);
}

__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_roots_count_kernel(int V, const int* __restrict__ vertex_label, int* __restrict__ block_count) {
  __shared__ int s_wave[kMcBlock / 64];
  const long long v = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  int total;
  compact_block_rank(v < V && vertex_label[v] == (int)v, s_wave, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_roots_scatter_kernel(int V, const int* __restrict__ vertex_label, const int* __restrict__ block_offset,
                                    const int* __restrict__ cnt_f, const int* __restrict__ cnt_v, int* __restrict__ comp_label,
                                    int* __restrict__ comp_faces, int* __restrict__ comp_vertices) {
  __shared__ int s_wave[kMcBlock / 64];
  const long long v = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  const bool root = v < V && vertex_label[v] == (int)v;
  int total;
  const int rank = compact_block_rank(root, s_wave, total);
  if (root) {
    const int c = block_offset[blockIdx.x] + rank;          // <= number of roots before v <= v < V
    comp_label[c] = (int)v;
    comp_faces[c] = cnt_f[v];
    comp_vertices[c] = cnt_v[v];
  }
}

// ---- filter: keep the vertices and faces of the components whose keep[label] is set, in their original order
// workspace: rank_v[V], rank_f[T] (rank of a kept element among the kept ones of its 256-block, -1 for a dropped one) and the two
// arrays of block offsets.
__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_filter_rank_kernel(int n, int V, const int* __restrict__ label, const unsigned char* __restrict__ keep,
                                  int* __restrict__ rank, int* __restrict__ block_count) {
  __shared__ int s_wave[kMcBlock / 64];
  const long long i = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  bool kept = false;
  if (i < n) {
    const int l = label[i];
    kept = (unsigned)l < (unsigned)V && keep[l] != 0;       // a face label of -1 (or anything else outside [0, V)) is never kept
  }
  int total;
  const int r = compact_block_rank(kept, s_wave, total);
  if (i < n) rank[i] = kept ? r : -1;
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__device__ __forceinline__ int mc_new_id(const int* __restrict__ rank, const int* __restrict__ block_offset, long long i) {
  const int r = rank[i];
  return r < 0 ? -1 : block_offset[i / kMcBlock] + r;
}

__global__ __launch_bounds__(kMcBlock)
void nerf_mesh_filter_emit_kernel(const float* __restrict__ vertices, const int* __restrict__ faces, int V, int T,
                                  const int* __restrict__ rank_v, const int* __restrict__ off_v, const int* __restrict__ rank_f,
                                  const int* __restrict__ off_f, float* __restrict__ out_vertices, int* __restrict__ out_faces,
                                  int* __restrict__ vertex_index) {
  const long long i = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  if (i < V) {
    const int nv = mc_new_id(rank_v, off_v, i);
    if (nv >= 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) out_vertices[3LL * nv + a] = vertices[3 * i + a];
      vertex_index[nv] = (int)i;
    }
  }
  if (i < T) {
    const int nf = mc_new_id(rank_f, off_f, i);
    if (nf >= 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int v = faces[3 * i + a];                      // in [0, V) when the faces are those that were counted; checked all the same
        out_faces[3LL * nf + a] = (unsigned)v < (unsigned)V ? mc_new_id(rank_v, off_v, v) : -1;
      }
    }
  }
}

inline long long mc_blocks(int64_t n) { return (n + kMcBlock - 1) / kMcBlock; }

int mc_sizes(const char* entry, int64_t n_vertices, int64_t n_faces) {
  if (n_vertices < 0 || n_faces < 0) return fail(NERF_ERR_INVALID_ARG, "%s: negative size", entry);
  if (n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL)
    return fail(NERF_ERR_INVALID_ARG, "%s: more than 2^31 - 1 vertices or faces", entry);
  return NERF_OK;
}
// The two workspaces (one buffer serves both: nerf_mesh_components_workspace_bytes is the larger).  nbv / nbf: 256-blocks of the
// vertices / faces
struct McComponentsWorkspace {
  long long nbv;
  int* parent; int* cnt_f; int* cnt_v; int* block;
  int64_t bytes;
  McComponentsWorkspace(const void* base, int64_t V) : nbv(mc_blocks(V)) {
    Carver c(base);
    parent = c.take<int>(V);
    cnt_f = c.take<int>(V);
    cnt_v = c.take<int>(V);
    block = c.take<int>(nbv);
    bytes = c.bytes();
  }
};
struct McFilterWorkspace {
  long long nbv, nbf;
  int* rank_v; int* rank_f; int* off_v; int* off_f;
  int64_t bytes;
  McFilterWorkspace(const void* base, int64_t V, int64_t T) : nbv(mc_blocks(V)), nbf(mc_blocks(T)) {
    Carver c(base);
    rank_v = c.take<int>(V);
    rank_f = c.take<int>(T);
    off_v = c.take<int>(nbv);
    off_f = c.take<int>(nbf);
    bytes = c.bytes();
  }
};

}  // namespace

extern "C" {

int64_t nerf_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
  if (mc_sizes("nerf_mesh_components_workspace_bytes", n_vertices, n_faces)) return -1;
  const int64_t a = McComponentsWorkspace(nullptr, n_vertices).bytes, b = McFilterWorkspace(nullptr, n_vertices, n_faces).bytes;
  return a > b ? a : b;
}

int32_t nerf_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, void* workspace, int32_t* vertex_label,
                             int32_t* face_label, int32_t* comp_label, int32_t* comp_faces, int32_t* comp_vertices,
                             int32_t* n_components, void* stream) {
  int rc = mc_sizes("nerf_mesh_components", n_vertices, n_faces);
  if (rc) return rc;
  if (!n_components) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mesh_components: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int V = (int)n_vertices, T = (int)n_faces;
  if (T > 0 && (!faces || !face_label)) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mesh_components: null argument");
  if (V == 0) {                                              // no vertex: every face is out of range
    if (hipMemsetAsync(n_components, 0, sizeof(int32_t), st) != hipSuccess ||
        (T > 0 && hipMemsetAsync(face_label, 0xff, T * sizeof(int32_t), st) != hipSuccess))
      return fail(NERF_ERR_HIP, "%s", "nerf_mesh_components: memset failed");
    return NERF_OK;
  }
  if (!workspace || !vertex_label || !comp_label || !comp_faces || !comp_vertices)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mesh_components: null argument");
  const McComponentsWorkspace L(workspace, V);
  const unsigned gv = (unsigned)L.nbv, gf = (unsigned)mc_blocks(T), gvf = gv > gf ? gv : gf;
  if ((rc = NERF_LAUNCH(nerf_mesh_init_kernel, dim3(gv), dim3(kMcBlock), st, V, L.parent, L.cnt_f, L.cnt_v))) return rc;
  if (T > 0) {
    if ((rc = NERF_LAUNCH(nerf_mesh_union_kernel, dim3(gf), dim3(kMcBlock), st, faces, T, V, L.parent))) return rc;
  }
  if ((rc = NERF_LAUNCH(nerf_mesh_flatten_kernel, dim3(gv), dim3(kMcBlock), st, V, L.parent, vertex_label))) return rc;
  if ((rc = NERF_LAUNCH(nerf_mesh_count_kernel, dim3(gvf), dim3(kMcBlock), st, faces, T, V, vertex_label, face_label, L.cnt_f,
                        L.cnt_v))) return rc;
  if ((rc = NERF_LAUNCH(nerf_mesh_roots_count_kernel, dim3(gv), dim3(kMcBlock), st, V, vertex_label, L.block))) return rc;
  if ((rc = NERF_LAUNCH(nerf_compact_scan_kernel, dim3(1), dim3(kScanThreads), st, L.block, L.nbv, n_components))) return rc;
  return NERF_LAUNCH(nerf_mesh_roots_scatter_kernel, dim3(gv), dim3(kMcBlock), st, V, vertex_label, L.block, L.cnt_f, L.cnt_v,
                     comp_label,
                     comp_faces, comp_vertices);
}

int32_t nerf_mesh_filter_count(const int32_t* vertex_label, const int32_t* face_label, const uint8_t* keep, int64_t n_vertices,
                               int64_t n_faces, void* workspace, int32_t* counts, void* stream) {
  int rc = mc_sizes("nerf_mesh_filter_count", n_vertices, n_faces);
  if (rc) return rc;
  if (!counts) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mesh_filter_count: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int V = (int)n_vertices, T = (int)n_faces;
  if (V == 0 || T == 0)                                      // (one of the two may stay 0: the scans below write the other)
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st) != hipSuccess) return fail(NERF_ERR_HIP, "%s", "nerf_mesh_filter_count: memset failed");
  if (V == 0) return NERF_OK;                                // no vertex, no label in range: nothing is kept
  if (!vertex_label || !keep || !workspace || (T > 0 && !face_label))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mesh_filter_count: null argument");
  const McFilterWorkspace L(workspace, V, T);
  if ((rc = NERF_LAUNCH(nerf_mesh_filter_rank_kernel, dim3((unsigned)L.nbv), dim3(kMcBlock), st, V, V, vertex_label, keep, L.rank_v,
                        L.off_v))) return rc;
  if ((rc = NERF_LAUNCH(nerf_compact_scan_kernel, dim3(1), dim3(kScanThreads), st, L.off_v, L.nbv, counts))) return rc;
  if (T > 0) {
    if ((rc = NERF_LAUNCH(nerf_mesh_filter_rank_kernel, dim3((unsigned)L.nbf), dim3(kMcBlock), st, T, V, face_label, keep, L.rank_f,
                          L.off_f))) return rc;
    if ((rc = NERF_LAUNCH(nerf_compact_scan_kernel, dim3(1), dim3(kScanThreads), st, L.off_f, L.nbf, counts + 1))) return rc;
  }
  return NERF_OK;
}

int32_t nerf_mesh_filter_emit(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const void* workspace,
                              float* out_vertices, int32_t* out_faces, int32_t* vertex_index, void* stream) {
  int rc = mc_sizes("nerf_mesh_filter_emit", n_vertices, n_faces);
  if (rc) return rc;
  const int V = (int)n_vertices, T = (int)n_faces;
  if (V == 0) return NERF_OK;
  if (!vertices || !workspace || !out_vertices || !vertex_index || (T > 0 && (!faces || !out_faces)))
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_mesh_filter_emit: null argument");
  const McFilterWorkspace L(workspace, V, T);
  const unsigned g = (unsigned)(L.nbv > L.nbf ? L.nbv : L.nbf);
  return NERF_LAUNCH(nerf_mesh_filter_emit_kernel, dim3(g), dim3(kMcBlock), (hipStream_t)stream, vertices, faces, V, T, L.rank_v,
                     L.off_v, L.rank_f, L.off_f, out_vertices, out_faces, vertex_index);
}

}  // extern "C"
