"""Geometry out of a trained network: the density on a grid and its iso-surface as a triangle mesh, the role of the
reference's src/utils/mesh_utils.py:8-46 (`extract_mesh(queryfn, level, bbox, output_path, N)`; cfg.level = 32.0,
cfg.resolution = 256, src/config/config.py:10-12).

The density comes from the fused MLP kernels (a grid line is a ray: nerf_mlp_forward_rays_density), the surface from the
nerf_isosurface_* kernels (marching tetrahedra, include/nerf_mi355x.h); DESIGN.md section 2.8 has the definitions and where
this departs from the reference's function, which is not runnable as written.  Vertex normals are the density gradient of the
fused data-gradient chain at the vertices (nerf_density_gradient).  Clean-up: the connected components of
the mesh and the filter that keeps whole components (nerf_mesh_components, nerf_mesh_filter_*), the role of
trimesh's split behind the reference's mesh_utils.py:45, and vertex colours from the network itself.  No CPU fallback: every number
comes out of a HIP kernel, torch only moves tensors (and normalises the [V,3] gradient of vertex_normals, takes the sigmoid of the
[V,3] colours, and picks rows of the per-component table).
"""
import collections
import numbers

import numpy as np
import torch

from . import _lib
from .network import Network, _reference_cfg

DEFAULT_LEVEL = 32.0
DEFAULT_RESOLUTION = 256
CHUNK_POINTS = 1 << 22          # default bound on the points per MLP launch of density_grid: 64 MiB of [P,4] fp32 scratch
QUERY_BATCH = 1 << 20           # points per call of a callable queryfn
GRADIENT_BLOCK_POINTS = 1 << 16 # default bound on the points per block of density_gradient: 1.3 GB of saved / gradient rows


def _shape3(N):
    dims = (N, N, N) if isinstance(N, numbers.Integral) and not isinstance(N, bool) else N
    try:
        dims = tuple(dims)
    except TypeError:
        raise ValueError(f"N must be an int or (nx, ny, nz), got {N!r}") from None
    if len(dims) != 3 or not all(isinstance(n, numbers.Integral) and not isinstance(n, bool) and n >= 1 for n in dims):
        raise ValueError(f"N must be an int or (nx, ny, nz) with every size >= 1, got {N!r}")
    dims = tuple(int(n) for n in dims)
    if dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
        raise ValueError(f"a grid of {dims} has more than 2^31 - 1 points")
    return dims


def _bbox(bbox):
    try:
        b = np.asarray(bbox, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"bbox must hold 6 numbers (min xyz, max xyz), got {bbox!r}") from None
    if b.shape != (6,) or not np.isfinite(b).all():
        raise ValueError(f"bbox must hold 6 finite numbers (min xyz, max xyz), got {bbox!r}")
    b = b.reshape(2, 3)
    if (b[1] < b[0]).any():
        raise ValueError(f"bbox max is below min: {bbox!r}")
    return b


def grid_axes(bbox, N):
    """The float64 coordinates of the grid points per axis: min + i * (max - min) / (n - 1) (min alone for n == 1), and the
    (origin, step) of the same grid."""
    dims, b = _shape3(N), _bbox(bbox)
    axes = [b[0, a] + np.arange(n, dtype=np.float64) * (b[1, a] - b[0, a]) / (n - 1) if n > 1 else np.array([b[0, a]])
            for a, n in enumerate(dims)]
    step = tuple(float((b[1, a] - b[0, a]) / (n - 1)) if n > 1 else 0.0 for a, n in enumerate(dims))
    return axes, tuple(float(v) for v in b[0]), step


def density_grid(net, bbox, N, model="fine", chunk_lines=None):
    """Pre-ReLU sigma of `net`'s coarse ("") or fine model on a grid: device tensor [nx, ny, nz] fp32.

    bbox: 6 numbers (min xyz, max xyz); N: an int or (nx, ny, nz), each >= 1.  Index i of an axis is at min + i (max - min) /
    (n - 1), evaluated in float64 and rounded once to fp32.  The grid lines along z are rays, rays_o = (x_i, y_j, 0), rays_d =
    (0, 0, 1), and the fp32 z coordinates are their shared depth table, so the kernels' o + d t is those coordinates exactly and
    the whole grid runs at the density-only rate of nerf_mlp_forward_rays_density, in every precision of net.precision.
    The nx * ny lines go through in chunks of `chunk_lines` (default: as many as keep a launch at 2^22 points, i.e. the [P,4]
    fp32 scratch at 64 MiB); the grid does not depend on the chunking."""
    if not isinstance(net, Network):
        raise TypeError("density_grid needs a nerf_replication_amd Network")
    if model not in ("", "fine"):
        raise ValueError(f'model must be "" (coarse) or "fine", got {model!r}')
    axes, _, _ = grid_axes(bbox, N)
    nx, ny, nz = (len(a) for a in axes)
    if chunk_lines is None:
        chunk_lines = max(1, CHUNK_POINTS // nz)
    if not isinstance(chunk_lines, numbers.Integral) or chunk_lines < 1:
        raise ValueError(f"chunk_lines must be a positive int, got {chunk_lines!r}")
    packed = net.packed(model)                     # raises for a network on the CPU
    dev = packed.device
    prec = _lib.PRECISIONS[net.precision]
    x, y, z = (torch.from_numpy(a.astype(np.float32)) for a in axes)
    lines = nx * ny
    rays_o = torch.zeros((lines, 3), dtype=torch.float32)
    rays_o[:, 0] = x[:, None].expand(nx, ny).reshape(-1)
    rays_o[:, 1] = y[None, :].expand(nx, ny).reshape(-1)
    rays_d = torch.zeros((lines, 3), dtype=torch.float32)
    rays_d[:, 2] = 1.0
    rays_o, rays_d, t = rays_o.to(dev), rays_d.to(dev), z.to(dev)
    grid = torch.empty((lines, nz), dtype=torch.float32, device=dev)
    raw = torch.empty((min(lines, int(chunk_lines)), nz, 4), dtype=torch.float32, device=dev)
    for l0 in range(0, lines, int(chunk_lines)):
        l1 = min(lines, l0 + int(chunk_lines))
        _lib.call("nerf_mlp_forward_rays_density", rays_o[l0:l1], rays_d[l0:l1], t, 0, l1 - l0, nz, packed, raw, prec)
        grid[l0:l1].copy_(raw[:l1 - l0, :, 3])
    return grid.view(nx, ny, nz)


def _field_layout(field):
    """(tensor whose first element is grid point (0,0,0), element stride, shape) of a dense [nx,ny,nz] grid or a [...,4] raw view."""
    if not isinstance(field, torch.Tensor):
        raise TypeError("field must be a torch tensor")
    if field.dtype != torch.float32:
        raise ValueError("field must be float32")
    if field.dim() == 4 and field.shape[3] == 4:              # raw [nx,ny,nz,4]: sigma is channel 3
        field = field[..., 3]
    if field.dim() != 3:
        raise ValueError("field must be [nx, ny, nz], or a raw buffer [nx, ny, nz, 4]")
    nx, ny, nz = (int(n) for n in field.shape)
    _shape3((max(nx, 1), max(ny, 1), max(nz, 1)))
    s = 1
    if min(nx, ny, nz) >= 2:                                    # (smaller grids have no cells: nothing is read)
        s = field.stride(2)
        if s < 1 or field.stride() != (ny * nz * s, nz * s, s):
            raise ValueError("field must be a dense grid or a channel of a contiguous [...,4] buffer (k fastest)")
    return field, int(s), (nx, ny, nz)


def _vec3(v, name):
    try:
        out = tuple(float(x) for x in v)
    except TypeError:
        raise ValueError(f"{name} must hold 3 numbers, got {v!r}") from None
    if len(out) != 3 or not all(np.isfinite(out)):
        raise ValueError(f"{name} must hold 3 finite numbers, got {v!r}")
    return out


def isosurface(field, level, origin, step):
    """Iso-surface {field = level} of a scalar grid as an indexed triangle mesh on the device:
    (vertices [V,3] float32, faces [T,3] int32).

    field: device tensor [nx,ny,nz] fp32 (point (i,j,k) at origin + (i,j,k) * step), or a raw buffer [nx,ny,nz,4] / any view of
    one of its channels (read in place with a stride of 4).  Marching tetrahedra on the Kuhn split of every cell; inside is
    field > level, faces wind so that their normal points from inside to outside; closed and manifold wherever the surface stays
    off the grid boundary, open where the boundary cuts it; repeatable to the byte (include/nerf_mi355x.h, nerf_isosurface_*).
    One host synchronisation: the two counts are read between the counting and the emitting pass."""
    field, stride, (nx, ny, nz) = _field_layout(field)
    level = float(level)
    origin, step = _vec3(origin, "origin"), _vec3(step, "step")
    if not field.is_cuda:
        raise _lib.NerfLibraryError("isosurface needs the field on a GPU (cuda) device; there is no CPU fallback")
    dev = field.device
    vertices = torch.empty((0, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((0, 3), dtype=torch.int32, device=dev)
    if min(nx, ny, nz) < 2:
        return vertices, faces
    nbytes = int(_lib.call("nerf_isosurface_workspace_bytes", nx, ny, nz))
    if nbytes < 0:
        raise _lib.NerfLibraryError(f"nerf_isosurface_workspace_bytes refused a grid of {nx} x {ny} x {nz} points")
    field = _lib.strided(field)                    # _field_layout has checked the layout that `stride` describes
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("nerf_isosurface_count", field, stride, nx, ny, nz, level, workspace, counts)
    n_v, n_t = (int(c) for c in counts.cpu())
    if n_v < 0 or n_t < 0:
        raise _lib.NerfLibraryError("isosurface: more than 2^31 - 1 vertices or triangles")
    if n_t == 0:
        return vertices, faces
    vertices = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
    _lib.call("nerf_isosurface_emit", field, stride, nx, ny, nz, level, origin, step, workspace, vertices, faces)
    return vertices, faces


def density_gradient(net, points, model="fine", positive_only=False, block_points=None):
    """(sigma [P], grad [P,3]) of `net`'s coarse ("") or fine model at explicit points [P,3] on the device: the pre-ReLU density and
    its spatial gradient, through nerf_density_gradient (include/nerf_mi355x.h, "geometry outputs"; net.precision 'f32' / 'f32x').
    Every point is a ray of one sample, rays_o = the point, rays_d = (0, 0, 1), t = 0, so the kernels' o + d t is the point itself.
    positive_only: grad is exactly zero wherever sigma <= 0.  The entry works in blocks of `block_points` points (default 2^16, about
    1.3 GB of scratch); the result does not depend on the blocking."""
    if not isinstance(net, Network):
        raise TypeError("density_gradient needs a nerf_replication_amd Network")
    if model not in ("", "fine"):
        raise ValueError(f'model must be "" (coarse) or "fine", got {model!r}')
    if block_points is None:
        block_points = GRADIENT_BLOCK_POINTS
    if isinstance(block_points, bool) or not isinstance(block_points, numbers.Integral) or block_points < 1:
        raise ValueError(f"block_points must be a positive int, got {block_points!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be a tensor [P,3]")
    packed = net.packed(model)                     # raises for a network on the CPU
    packed_bwd = net.packed_bwd(model)             # raises for an fp16 precision
    dev = packed.device
    pts = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    P = pts.shape[0]
    sigma = torch.empty((P,), dtype=torch.float32, device=dev)
    grad = torch.empty((P, 3), dtype=torch.float32, device=dev)
    if P == 0:
        return sigma, grad
    rays_d = torch.zeros((P, 3), dtype=torch.float32, device=dev)
    rays_d[:, 2] = 1.0
    t = torch.zeros(1, dtype=torch.float32, device=dev)
    rows = (min(int(block_points), P) + 31) // 32 * 32
    ws = torch.empty(int(_lib.call("nerf_density_gradient_point_bytes")) * rows, dtype=torch.uint8, device=dev)
    _lib.call("nerf_density_gradient", pts, rays_d, t, 0, P, 1, packed, packed_bwd, int(bool(positive_only)), sigma, grad,
              _lib.PRECISIONS[net.precision], ws, ws.numel())
    return sigma, grad


def vertex_normals(net, vertices, model="fine"):
    """Unit outward normals [V,3] of an iso-surface of `net`'s density at its vertices [V,3]: -grad sigma / |grad sigma| (density
    falls towards the outside), the gradient from density_gradient (every point, whatever the sign of sigma).  A vertex with a zero
    (or non-finite) gradient gets the zero vector.  The gradient comes out of the HIP chain; the normalisation of the [V,3] result
    is three torch operations."""
    _, g = density_gradient(net, vertices, model=model, positive_only=False)
    nrm = g.norm(dim=-1, keepdim=True)
    ok = torch.isfinite(nrm) & (nrm > 0)
    return torch.where(ok, -g / torch.where(ok, nrm, torch.ones_like(nrm)), torch.zeros_like(g))


ComponentTable = collections.namedtuple("ComponentTable", ["label", "faces", "vertices"])
ComponentTable.__doc__ = """One row per connected component, ascending label: its label (smallest vertex id), face count and vertex
count; three device tensors [C] int32."""


def _count(x, name):
    if x is None:
        return None
    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or x < 0:
        raise ValueError(f"{name} must be a non-negative int, got {x!r}")
    return int(x)


def _mesh_arrays(vertices, faces):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("faces must be an integer tensor [T,3]")
    if vertices is not None and (not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or
                                 not vertices.is_floating_point()):
        raise ValueError("vertices must be a floating-point tensor [V,3]")


class _Components:
    """The labels and the table of one mesh, with the workspace they share with the filter."""

    def __init__(self, faces, n_vertices):
        if not faces.is_cuda:
            raise _lib.NerfLibraryError("mesh_components needs the faces on a GPU (cuda) device; there is no CPU fallback")
        dev = faces.device
        self.faces = faces.detach().to(torch.int32).contiguous()
        self.V, self.T = V, T = int(n_vertices), int(faces.shape[0])
        nbytes = int(_lib.call("nerf_mesh_components_workspace_bytes", V, T))
        if nbytes < 0:
            raise _lib.NerfLibraryError(f"nerf_mesh_components_workspace_bytes refused {V} vertices and {T} faces")
        self.workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        self.vertex_label = torch.empty(V, dtype=torch.int32, device=dev)
        self.face_label = torch.empty(T, dtype=torch.int32, device=dev)
        rows = torch.empty((3, V), dtype=torch.int32, device=dev)
        n_comp = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call("nerf_mesh_components", self.faces, T, V, self.workspace, self.vertex_label, self.face_label, *rows, n_comp)
        C = int(n_comp.item())
        self.table = ComponentTable(rows[0, :C], rows[1, :C], rows[2, :C])

    def select(self, min_triangles, keep_largest):
        """keep [V] uint8, indexed by label: the rows of the table (C rows, C << V) that pass, as a few torch operations."""
        label, n_faces, _ = self.table
        ok = torch.ones_like(label, dtype=torch.bool)
        if min_triangles is not None:
            ok &= n_faces >= min_triangles
        if keep_largest is not None:
            order = torch.sort(-n_faces.to(torch.int64), stable=True).indices        # most faces first, ties by the smaller label
            top = torch.zeros_like(ok)
            top[order[:keep_largest]] = True
            ok &= top
        keep = torch.zeros(self.V, dtype=torch.uint8, device=label.device)
        keep[label[ok].to(torch.int64)] = 1
        return keep

    def filter(self, vertices, keep):
        dev = self.faces.device
        V, T = self.V, self.T
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.call("nerf_mesh_filter_count", self.vertex_label, self.face_label, keep, V, T, self.workspace, counts)
        n_v, n_t = (int(c) for c in counts.cpu())
        out_v = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
        index = torch.empty(n_v, dtype=torch.int32, device=dev)
        if n_v > 0:
            _lib.call("nerf_mesh_filter_emit", vertices, self.faces, V, T, self.workspace, out_v, out_f, index)
        return out_v, out_f, index


def mesh_components(faces, n_vertices):
    """Connected components of an indexed triangle mesh on the device: (vertex_label [V] int32, face_label [T] int32, table).

    faces: device tensor [T,3] of vertex ids below n_vertices.  Two vertices are connected when a face names both; the label of a
    vertex is the smallest vertex id of its component, the label of a face that of its first vertex; a face with an index outside
    [0, V) joins nothing and has the label -1.  table: ComponentTable(label, faces, vertices), three [C] tensors, ascending label; a
    vertex no face names is a component with 0 faces.  Lock-free union-find in HIP (nerf_mesh_components, include/nerf_mi355x.h);
    repeatable to the byte.  One host synchronisation: the number of components."""
    _mesh_arrays(None, faces)
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, numbers.Integral) or not 0 <= n_vertices <= 2 ** 31 - 1:
        raise ValueError(f"n_vertices must be an int in [0, 2^31 - 1], got {n_vertices!r}")
    if faces.shape[0] > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 faces")
    c = _Components(faces, n_vertices)
    return c.vertex_label, c.face_label, c.table


def _filter_arguments(min_triangles, keep_largest, required):
    min_triangles, keep_largest = _count(min_triangles, "min_triangles"), _count(keep_largest, "keep_largest")
    if required and min_triangles is None and keep_largest is None:
        raise ValueError("filter_components needs min_triangles, keep_largest or both")
    return min_triangles, keep_largest


def filter_components(vertices, faces, min_triangles=None, keep_largest=None):
    """Drop whole connected components of a mesh: (vertices' [V',3] float32, faces' [T',3] int32, vertex_index [V'] int32).

    min_triangles=m keeps the components with at least m faces; keep_largest=k keeps the k components with the most faces, ties
    going to the smaller label (the smaller lowest vertex id); with both, a component must pass both.  The kept vertices and faces
    stay in their original order, faces re-indexed; vertex_index holds the old id of every new vertex (vertices' is
    vertices[vertex_index]; gather normals or colours with it).  Faces with an index outside [0, V) are dropped.  The components,
    the counting and the copying are HIP (nerf_mesh_components, nerf_mesh_filter_*); choosing rows of the per-component table is a
    few torch operations.  Two host synchronisations: the number of components, and the two counts."""
    min_triangles, keep_largest = _filter_arguments(min_triangles, keep_largest, True)
    _mesh_arrays(vertices, faces)
    if vertices.shape[0] > 2 ** 31 - 1 or faces.shape[0] > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 vertices or faces")
    if not vertices.is_cuda or vertices.device != faces.device:
        raise _lib.NerfLibraryError("filter_components needs vertices and faces on one GPU (cuda) device; there is no CPU fallback")
    comps = _Components(faces, vertices.shape[0])
    return comps.filter(vertices.detach().to(torch.float32).contiguous(), comps.select(min_triangles, keep_largest))


def _head_on(normals):
    """The direction of travel of a ray that meets the surface head-on from outside: -normal, (0, 0, 1) where the normal is zero."""
    ahead = torch.tensor([0.0, 0.0, 1.0], dtype=normals.dtype, device=normals.device)
    return torch.where((normals == 0).all(dim=-1, keepdim=True), ahead, -normals)


def vertex_colors(net, vertices, viewdirs=None, model="fine"):
    """Colours [V,3] fp32 in [0,1] of `net`'s coarse ("") or fine model at the vertices [V,3]: sigmoid(raw[:, :3]) of Network.forward
    (inputs [V,1,3], viewdirs [V,3], inference path, every precision of net.precision).  viewdirs=None looks at every vertex head-on
    from outside: the direction of travel is -vertex_normals(net, vertices, model) ((0, 0, 1) where the normal is the zero vector;
    the normals need net.precision 'f32' / 'f32x').  The raw values come out of the fused MLP kernel; the sigmoid of the [V,3] result
    is one torch operation."""
    if not isinstance(net, Network):
        raise TypeError("vertex_colors needs a nerf_replication_amd Network")
    if model not in ("", "fine"):
        raise ValueError(f'model must be "" (coarse) or "fine", got {model!r}')
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertices must be a tensor [V,3]")
    if viewdirs is not None and (not isinstance(viewdirs, torch.Tensor) or viewdirs.shape != vertices.shape):
        raise ValueError(f"viewdirs must be a tensor of the vertices' shape {tuple(vertices.shape)}")
    dev = net.packed(model).device                 # raises for a network on the CPU
    pts = vertices.detach().to(device=dev, dtype=torch.float32).contiguous()
    if pts.shape[0] == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    if viewdirs is None:
        viewdirs = _head_on(vertex_normals(net, pts, model=model))
    dirs = viewdirs.detach().to(device=dev, dtype=torch.float32).contiguous()
    with torch.no_grad():
        raw = net.forward(pts[:, None, :], dirs, None, model=model)
    return torch.sigmoid(raw[:, 0, :3])


def write_ply(path, vertices, faces, normals=None):
    """Binary little-endian PLY: `float` x y z per vertex (followed by `float` nx ny nz when `normals` [V,3] is given), `uchar int`
    index lists per face.  write_ply_colors writes colours as well."""
    _write_ply(path, vertices, faces, normals, None)


def write_ply_colors(path, vertices, faces, normals=None, colors=None):
    """write_ply with vertex colours: `uchar` red green blue per vertex, behind nx ny nz when both are given.  colors [V,3] are floats
    in [0,1], written as floor(clip(c, 0, 1) * 255 + 0.5), exactly (evaluated in float64; NaN gives 0).  With colors=None the bytes are
    write_ply's.  (A function of its own: write_ply's parameter list is part of the tested surface and stays as it is.)"""
    _write_ply(path, vertices, faces, normals, colors)


def _write_ply(path, vertices, faces, normals, colors):
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4")
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("write_ply needs vertices [V,3] and faces [T,3]")
    n_v = len(v)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        nv = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype="<f4")
        if nv.shape != v.shape:
            raise ValueError(f"write_ply needs normals of the vertices' shape {v.shape}, got {nv.shape}")
        v = np.ascontiguousarray(np.concatenate([v, nv], axis=1))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        c = np.asarray(torch.as_tensor(colors).detach().cpu().numpy(), dtype=np.float64)
        if c.shape != (n_v, 3):
            raise ValueError(f"write_ply_colors needs colors of the vertices' shape {(n_v, 3)}, got {c.shape}")
        vrec = np.empty(n_v, dtype=np.dtype([("f", "<f4", (v.shape[1],)), ("c", "u1", (3,))]))      # packed: no padding
        vrec["f"], vrec["c"] = v, np.floor(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        v = vrec
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {n_v}\n" + props +
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    rec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, f
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def _query_grid(queryfn, axes, device):
    """The reference's protocol: queryfn(xyz [n,3] on the GPU) -> [..., 0] is the density; explicit grid points in batches."""
    nx, ny, nz = (len(a) for a in axes)
    x, y, z = (torch.from_numpy(a.astype(np.float32)).to(device) for a in axes)
    grid = torch.empty(nx * ny * nz, dtype=torch.float32, device=device)
    per = max(1, QUERY_BATCH // (ny * nz))                      # whole x-slabs per call
    with torch.no_grad():
        for i0 in range(0, nx, per):
            i1 = min(nx, i0 + per)
            pts = torch.stack(torch.meshgrid(x[i0:i1], y, z, indexing="ij"), dim=-1).reshape(-1, 3)
            out = queryfn(pts)
            sigma = out[..., 0].reshape(-1).to(torch.float32)
            if sigma.numel() != pts.shape[0]:
                raise ValueError(f"queryfn returned {sigma.numel()} densities for {pts.shape[0]} points")
            grid[i0 * ny * nz:i1 * ny * nz] = sigma
    return grid.view(nx, ny, nz)


def extract_mesh(queryfn, level=None, bbox=None, output_path="test.ply", N=None, normals=None, min_triangles=None, keep_largest=None,
                 colors=None):
    """The reference's extract_mesh (src/utils/mesh_utils.py:8-46), same argument order: density on an N^3 grid over `bbox`, the
    iso-surface at `level`, written to `output_path` as a PLY; returns (vertices, faces) on the device.
    normals: None -- positions and faces only (the bytes are what they always were); True -- vertex_normals of the fine model are
    written with the vertices (queryfn must be a Network); an array [V,3] is passed through to write_ply as it is.
    min_triangles / keep_largest: filter_components between the surface and the normals / colours (floaters are dropped before
    anything is evaluated at them); the filtered (vertices, faces) are written and returned.  colors: None -- no colours; True --
    vertex_colors of the fine model, each vertex seen head-on from outside (queryfn must be a Network); an array [V,3] in [0,1] is
    passed through to write_ply_colors.  Arrays must match the vertices that are written.  With the defaults the result and the file are what
    they always were.

    queryfn: a Network (the fast path: density_grid on its fine model), a HashField (its density on the grid points; normals=True /
    colors=True are its vertex_normals / vertex_colors, and bbox=None is the field's own box), or a callable taking xyz [n,3] on
    the GPU whose result's [..., 0] is the density (the reference's protocol; evaluated on explicit grid points in batches).  level and N
    default to cfg.level / cfg.resolution inside the reference, else 32.0 / 256.  Arguments are checked before any GPU work."""
    cfg = _reference_cfg()
    if level is None:
        level = getattr(cfg, "level", DEFAULT_LEVEL) if cfg is not None else DEFAULT_LEVEL
    if N is None:
        N = getattr(cfg, "resolution", DEFAULT_RESOLUTION) if cfg is not None else DEFAULT_RESOLUTION
    from .hashfield import HashField
    field = queryfn if isinstance(queryfn, HashField) else None
    if not isinstance(queryfn, Network) and not callable(queryfn):
        raise TypeError("queryfn must be a Network or a callable xyz [n,3] -> [..., 0] density")
    if isinstance(level, bool) or not isinstance(level, numbers.Real) or not np.isfinite(level):
        raise ValueError(f"level must be a finite number, got {level!r}")
    if bbox is None and field is not None:
        bbox = field.bbox
    if bbox is None:
        raise ValueError("bbox is required: 6 numbers (min xyz, max xyz)")
    if not isinstance(output_path, (str, bytes)) and not hasattr(output_path, "__fspath__"):
        raise TypeError(f"output_path must be a path, got {output_path!r}")
    if normals is True and not isinstance(queryfn, Network) and field is None:
        raise TypeError("normals=True needs a Network as queryfn (vertex_normals); pass an array [V,3] otherwise")
    if normals is False:
        normals = None
    if colors is True and not isinstance(queryfn, Network) and field is None:
        raise TypeError("colors=True needs a Network as queryfn (vertex_colors); pass an array [V,3] otherwise")
    if colors is False:
        colors = None
    min_triangles, keep_largest = _filter_arguments(min_triangles, keep_largest, False)
    axes, origin, step = grid_axes(bbox, N)
    if isinstance(queryfn, Network):
        grid = density_grid(queryfn, bbox, N, model="fine")
    elif field is not None:                            # a HashField: its density on explicit grid points, on the field's device
        grid = _query_grid(field.density, axes, field.wbounds.device)
    else:
        if not torch.cuda.is_available():
            raise _lib.NerfLibraryError("extract_mesh needs a GPU; there is no CPU fallback")
        grid = _query_grid(queryfn, axes, torch.device("cuda", torch.cuda.current_device()))
    vertices, faces = isosurface(grid, level, origin, step)
    if min_triangles is not None or keep_largest is not None:
        vertices, faces, _ = filter_components(vertices, faces, min_triangles, keep_largest)
    made_normals = normals is True
    if made_normals:
        normals = field.vertex_normals(vertices) if field is not None else vertex_normals(queryfn, vertices, model="fine")
    if colors is True:                             # (the normals just computed are the ones vertex_colors would compute again)
        head_on = _head_on(normals) if made_normals else None
        colors = field.vertex_colors(vertices, head_on) if field is not None else vertex_colors(queryfn, vertices, head_on, model="fine")
    _write_ply(output_path, vertices, faces, normals, colors)
    return vertices, faces
