// Iso-surface extraction: marching tetrahedra over the six-tetrahedra (Kuhn) split of every grid cell (DESIGN.md section 2.8).
//
// Grid point (i, j, k) has the linear id g = (i*ny + j)*nz + k and the value field[g * stride]; a cell is named by its lowest
// corner.  Every edge of the split runs from a point p to p + e, e in {0,1}^3 \ 0: seven edge types t = 4 ex + 2 ey + ez, owned
// by p.  One 32-bit workspace word per point:
//     bits 0..6   crossing mask: bit t-1 set iff p + e is in the grid and inside(p) != inside(p + e)     (inside: f > level)
//     bits 7..17  number of crossed edges owned by the points before p in its 256-point block           (<= 255*7)
//     bits 18..29 number of triangles of the cells before p in its block                                (<= 255*12)
//     bit 30      inside(p)
// plus two int32 per block: its vertex and triangle totals, turned into exclusive offsets by the scan.  The emit pass takes the
// whole topology from these words (the field gives only the interpolation values), so what it writes stays inside the counted
// rows whatever the field holds by then.  Vertex ids ascend with (owner id, edge type), triangles with (cell id, tetrahedron,
// triangle); nothing is atomic, so two runs write the same bytes.
#include "nerf_host.h"
#include "nerf_isosurface_table.inc"
#include "nerf_scan.hip.inc"

namespace {

constexpr int kIsoBlock = kRankBlock;          // iso_block_exclusive (nerf_scan.hip.inc)

struct IsoGrid {
  int nx, ny, nz;
  long long n, stride;
};

// (i, j, k) of point g and whether g + corner o is in the grid
__device__ __forceinline__ void iso_ijk(const IsoGrid& G, long long g, int& i, int& j, int& k) {
  k = (int)(g % G.nz);
  const long long r = g / G.nz;
  j = (int)(r % G.ny);
  i = (int)(r / G.ny);
}
__device__ __forceinline__ long long iso_corner_offset(const IsoGrid& G, int o) {
  return (long long)((o >> 2) & 1) * G.ny * G.nz + (long long)((o >> 1) & 1) * G.nz + (o & 1);
}

__global__ __launch_bounds__(kIsoBlock)
void nerf_isosurface_count_kernel(const float* __restrict__ field, IsoGrid G, float level, unsigned* __restrict__ words,
                                  int* __restrict__ block_v, int* __restrict__ block_t) {
  __shared__ int s_wave[kIsoBlock / 64];
  const long long g = (long long)blockIdx.x * kIsoBlock + threadIdx.x;
  unsigned mask = 0, in0 = 0;
  int ntri = 0;
  if (g < G.n) {
    int i, j, k;
    iso_ijk(G, g, i, j, k);
    in0 = field[g * G.stride] > level ? 1u : 0u;
    unsigned corners = in0;                       // bit o: corner o inside
#pragma unroll
    for (int o = 1; o < 8; ++o) {
      const bool there = i + ((o >> 2) & 1) < G.nx && j + ((o >> 1) & 1) < G.ny && k + (o & 1) < G.nz;
      if (there) {
        const unsigned in = field[(g + iso_corner_offset(G, o)) * G.stride] > level ? 1u : 0u;
        corners |= in << o;
        mask |= (in ^ in0) << (o - 1);
      }
    }
    if (i + 1 < G.nx && j + 1 < G.ny && k + 1 < G.nz) ntri = kIsoCellTris[corners];
  }
  const int mine = __popc(mask) | (ntri << 16);
  int total;
  const int before = iso_block_exclusive(mine, s_wave, total);        // <= 1792 | 3072 << 16: the halves cannot carry
  if (g < G.n) words[g] = mask | (unsigned)(before & 0xffff) << 7 | (unsigned)(before >> 16) << 18 | in0 << 30;
  if (threadIdx.x == 0) {
    block_v[blockIdx.x] = total & 0xffff;
    block_t[blockIdx.x] = total >> 16;
  }
}

// block totals -> exclusive offsets in place, counts = (vertices, triangles); one workgroup, as nerf_compact_scan_kernel.  The
// sums are 64-bit: totals beyond int32 give counts = (-1, -1) (and meaningless offsets: nerf_isosurface_emit must not follow).
struct IsoSums {                              // (vertices, triangles)
  long long v, t;
  __device__ IsoSums operator+(const IsoSums& o) const { return {v + o.v, t + o.t}; }
  __device__ IsoSums operator-(const IsoSums& o) const { return {v - o.v, t - o.t}; }
};
__global__ __launch_bounds__(kScanThreads)
void nerf_isosurface_scan_kernel(int* __restrict__ block_v, int* __restrict__ block_t, long long n_blocks, int* __restrict__ counts) {
  __shared__ IsoSums s_sum[kScanThreads];
  const IsoSums total = workgroup_scan(n_blocks, s_sum, [&](long long b) { return IsoSums{block_v[b], block_t[b]}; },
                                       [&](long long b, IsoSums pos) { block_v[b] = (int)pos.v; block_t[b] = (int)pos.t; });
  if (threadIdx.x == 0) {
    const bool fits = total.v <= 0x7fffffffLL && total.t <= 0x7fffffffLL;
    counts[0] = fits ? (int)total.v : -1;
    counts[1] = fits ? (int)total.t : -1;
  }
}

struct IsoFrame { double origin[3], step[3]; };

// fp32 coordinate of grid index `idx` on one axis: one float64 product and sum, rounded once
__device__ __forceinline__ float iso_coord(const IsoFrame& F, int axis, int idx) {
  return (float)__dadd_rn(F.origin[axis], __dmul_rn((double)idx, F.step[axis]));
}

__device__ __forceinline__ int iso_vertex_id(const IsoGrid& G, const unsigned* __restrict__ words, const int* __restrict__ block_v,
                                             long long cell, int ref) {
  const long long p = cell + iso_corner_offset(G, ref >> 3);
  const unsigned w = words[p];
  return block_v[p / kIsoBlock] + (int)((w >> 7) & 0x7ffu) + __popc(w & ((1u << ((ref & 7) - 1)) - 1u));
}

__global__ __launch_bounds__(kIsoBlock)
void nerf_isosurface_emit_kernel(const float* __restrict__ field, IsoGrid G, float level, IsoFrame F, const unsigned* __restrict__ words,
                                 const int* __restrict__ block_v, const int* __restrict__ block_t, float* __restrict__ vertices,
                                 int* __restrict__ triangles) {
  const long long g = (long long)blockIdx.x * kIsoBlock + threadIdx.x;
  if (g >= G.n) return;
  const unsigned w = words[g];
  const unsigned mask = w & 0x7fu;
  if (mask == 0) return;             // no crossed edge at this point: no vertex, and its cell (if any) has one sign throughout
  int idx[3];
  iso_ijk(G, g, idx[0], idx[1], idx[2]);

  // ---- the vertices this point owns: on the edge (a, b) = (g, g + e), tau = (level - f_a) / (f_b - f_a), x_a + tau (x_b - x_a)
  {
    const float fa = field[g * G.stride];
    float xa[3], xb[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { xa[a] = iso_coord(F, a, idx[a]); xb[a] = iso_coord(F, a, idx[a] + 1); }
    long long v = (long long)block_v[blockIdx.x] + ((w >> 7) & 0x7ffu);
#pragma unroll
    for (int t = 1; t < 8; ++t) {
      if (!((mask >> (t - 1)) & 1u)) continue;
      const float fb = field[(g + iso_corner_offset(G, t)) * G.stride];
      const float tau = __fdiv_rn(__fsub_rn(level, fa), __fsub_rn(fb, fa));
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float other = ((t >> (2 - a)) & 1) ? xb[a] : xa[a];
        vertices[3 * v + a] = __fadd_rn(xa[a], __fmul_rn(tau, __fsub_rn(other, xa[a])));
      }
      ++v;
    }
  }

  // ---- the triangles of the cell whose lowest corner this point is
  if (!(idx[0] + 1 < G.nx && idx[1] + 1 < G.ny && idx[2] + 1 < G.nz)) return;
  const unsigned in0 = (w >> 30) & 1u;
  const unsigned corners = in0 | ((in0 ? ~mask : mask) & 0x7fu) << 1;       // corner o inside = inside(g) xor crossed(edge type o)
  long long t_out = (long long)block_t[blockIdx.x] + ((w >> 18) & 0xfffu);
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    int s = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) s |= (int)((corners >> kIsoTetCorner[q][m]) & 1u) << m;
    const int nt = kIsoTetTris[q][s];
    for (int e = 0; e < 3 * nt; ++e)
      triangles[3 * t_out + e] = iso_vertex_id(G, words, block_v, g, kIsoTetEdges[q][s][e]);
    t_out += nt;
  }
}

// 0: sizes fine; the grid as IsoGrid.  More than 2^31 - 1 points: point, vertex and triangle ids are int32
int iso_sizes(const char* entry, int32_t nx, int32_t ny, int32_t nz, int64_t stride, IsoGrid& G) {
  if (nx < 0 || ny < 0 || nz < 0 || stride < 1) return fail(NERF_ERR_INVALID_ARG, "%s: bad size", entry);
  const long long n = (long long)nx * ny;              // < 2^62
  if (nz > 0 && n > 0x7fffffffLL / nz) return fail(NERF_ERR_INVALID_ARG, "%s: more than 2^31 - 1 grid points", entry);
  G.nx = nx; G.ny = ny; G.nz = nz; G.n = n * nz; G.stride = stride;
  return NERF_OK;
}
inline bool iso_no_cells(const IsoGrid& G) { return G.nx < 2 || G.ny < 2 || G.nz < 2; }

// The workspace: one word per grid point, then the vertex and the triangle totals of every 256-point block
struct IsoWorkspace {
  long long n_blocks;
  unsigned* words; int* block_v; int* block_t;
  int64_t bytes;
  IsoWorkspace(const void* base, const IsoGrid& G) : n_blocks((G.n + kIsoBlock - 1) / kIsoBlock) {
    Carver c(base);
    words = c.take<unsigned>(G.n);
    block_v = c.take<int>(n_blocks);
    block_t = c.take<int>(n_blocks);
    bytes = c.bytes();
  }
};

}  // namespace

extern "C" {

int64_t nerf_isosurface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  IsoGrid G;
  if (iso_sizes("nerf_isosurface_workspace_bytes", nx, ny, nz, 1, G)) return -1;
  return IsoWorkspace(nullptr, G).bytes;
}

int32_t nerf_isosurface_count(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace,
                              int32_t* counts, void* stream) {
  IsoGrid G;
  int rc = iso_sizes("nerf_isosurface_count", nx, ny, nz, stride, G);
  if (rc) return rc;
  if (!counts) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_isosurface_count: null argument");
  hipStream_t st = (hipStream_t)stream;
  if (iso_no_cells(G)) {
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st) != hipSuccess) return fail(NERF_ERR_HIP, "%s", "nerf_isosurface_count: memset failed");
    return NERF_OK;
  }
  if (!field || !workspace) return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_isosurface_count: null argument");
  const IsoWorkspace w(workspace, G);
  if ((rc = NERF_LAUNCH(nerf_isosurface_count_kernel, dim3((unsigned)w.n_blocks), dim3(kIsoBlock), st, field, G, level, w.words,
                        w.block_v, w.block_t)))
    return rc;
  return NERF_LAUNCH(nerf_isosurface_scan_kernel, dim3(1), dim3(kScanThreads), st, w.block_v, w.block_t, w.n_blocks, counts);
}

int32_t nerf_isosurface_emit(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level, const double origin[3],
                             const double step[3], const void* workspace, float* vertices, int32_t* triangles, void* stream) {
  IsoGrid G;
  int rc = iso_sizes("nerf_isosurface_emit", nx, ny, nz, stride, G);
  if (rc) return rc;
  if (iso_no_cells(G)) return NERF_OK;
  if (!field || !origin || !step || !workspace || !vertices || !triangles)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_isosurface_emit: null argument");
  const IsoWorkspace w(workspace, G);
  IsoFrame F;
  for (int a = 0; a < 3; ++a) { F.origin[a] = origin[a]; F.step[a] = step[a]; }
  return NERF_LAUNCH(nerf_isosurface_emit_kernel, dim3((unsigned)w.n_blocks), dim3(kIsoBlock), (hipStream_t)stream, field, G, level, F,
                     w.words, w.block_v, w.block_t, vertices, triangles);
}

}  // extern "C"
