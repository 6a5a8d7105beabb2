// Iso-surface extraction: marching tetrahedra over the six-tetrahedra (Kuhn) split of every grid cell (DESIGN.md section 2.8).
// Included at the end of nerf_kernels.hip (uses its fail / check_launch / align256).
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
#include "nerf_isosurface_table.inc"

namespace {

constexpr int kIsoBlock = 256;

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

// exclusive rank of `v` among the block's threads (v < 2^16 per thread; two 16-bit fields are scanned as one int by the caller)
__device__ __forceinline__ int iso_block_exclusive(int v, int* s_wave, int& block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kIsoBlock / 64; ++w) {
    const int c = s_wave[w];
    if (w < wave) before += c;
    total += c;
  }
  block_total = total;
  return before + inc - v;
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
__global__ __launch_bounds__(1024)
void nerf_isosurface_scan_kernel(int* __restrict__ block_v, int* __restrict__ block_t, long long n_blocks, int* __restrict__ counts) {
  __shared__ long long s_v[1024], s_t[1024];
  const int tid = threadIdx.x;
  const long long per = (n_blocks + 1023) / 1024;
  const long long b0 = tid * per < n_blocks ? tid * per : n_blocks, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
  long long cv = 0, ct = 0;
  for (long long b = b0; b < b1; ++b) { cv += block_v[b]; ct += block_t[b]; }
  s_v[tid] = cv; s_t[tid] = ct;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {                 // inclusive Hillis-Steele scan
    const long long v = tid >= d ? s_v[tid - d] : 0, t = tid >= d ? s_t[tid - d] : 0;
    __syncthreads();
    s_v[tid] += v; s_t[tid] += t;
    __syncthreads();
  }
  long long pv = s_v[tid] - cv, pt = s_t[tid] - ct;
  for (long long b = b0; b < b1; ++b) {
    const int v = block_v[b], t = block_t[b];
    block_v[b] = (int)pv; block_t[b] = (int)pt;
    pv += v; pt += t;
  }
  if (tid == 1023) {
    const bool fits = s_v[1023] <= 0x7fffffffLL && s_t[1023] <= 0x7fffffffLL;
    counts[0] = fits ? (int)s_v[1023] : -1;
    counts[1] = fits ? (int)s_t[1023] : -1;
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
inline long long iso_blocks(const IsoGrid& G) { return (G.n + kIsoBlock - 1) / kIsoBlock; }

}  // namespace

extern "C" {

int64_t nerf_isosurface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  IsoGrid G;
  if (iso_sizes("nerf_isosurface_workspace_bytes", nx, ny, nz, 1, G)) return -1;
  return align256(G.n * (int64_t)sizeof(unsigned)) + 2 * align256(iso_blocks(G) * (int64_t)sizeof(int));
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
  const long long n_blocks = iso_blocks(G);
  unsigned* words = (unsigned*)workspace;
  int* block_v = (int*)((char*)workspace + align256(G.n * (int64_t)sizeof(unsigned)));
  int* block_t = (int*)((char*)block_v + align256(n_blocks * (int64_t)sizeof(int)));
  hipLaunchKernelGGL(nerf_isosurface_count_kernel, dim3((unsigned)n_blocks), dim3(kIsoBlock), 0, st, field, G, level, words, block_v, block_t);
  rc = check_launch("nerf_isosurface_count_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(nerf_isosurface_scan_kernel, dim3(1), dim3(1024), 0, st, block_v, block_t, n_blocks, counts);
  return check_launch("nerf_isosurface_scan_kernel");
}

int32_t nerf_isosurface_emit(const float* field, int64_t stride, int32_t nx, int32_t ny, int32_t nz, float level, const double origin[3],
                             const double step[3], const void* workspace, float* vertices, int32_t* triangles, void* stream) {
  IsoGrid G;
  int rc = iso_sizes("nerf_isosurface_emit", nx, ny, nz, stride, G);
  if (rc) return rc;
  if (iso_no_cells(G)) return NERF_OK;
  if (!field || !origin || !step || !workspace || !vertices || !triangles)
    return fail(NERF_ERR_INVALID_ARG, "%s", "nerf_isosurface_emit: null argument");
  const long long n_blocks = iso_blocks(G);
  const unsigned* words = (const unsigned*)workspace;
  const int* block_v = (const int*)((const char*)workspace + align256(G.n * (int64_t)sizeof(unsigned)));
  const int* block_t = (const int*)((const char*)block_v + align256(n_blocks * (int64_t)sizeof(int)));
  IsoFrame F;
  for (int a = 0; a < 3; ++a) { F.origin[a] = origin[a]; F.step[a] = step[a]; }
  hipLaunchKernelGGL(nerf_isosurface_emit_kernel, dim3((unsigned)n_blocks), dim3(kIsoBlock), 0, (hipStream_t)stream, field, G, level, F, words,
                     block_v, block_t, vertices, triangles);
  return check_launch("nerf_isosurface_emit_kernel");
}

}  // extern "C"
