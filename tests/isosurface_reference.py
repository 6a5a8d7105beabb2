"""NumPy float32 restatement of the iso-surface definitions of DESIGN.md section 2.8 (include/nerf_mi355x.h, nerf_isosurface_*),
every operation separately rounded, for the GPU tests to compare with bit for bit.  A helper, not a test.

Written independently of the kernel's case table (tools/gen_isosurface_table.py): the tetrahedra and their sign cases are
enumerated here directly, and the winding comes from the tetrahedron's signed volume instead of the generator's midpoint
geometry:
  * one vertex L apart from the other three r0 < r1 < r2 (tetrahedron vertex numbers): with d = det(r0 - L, r1 - L, r2 - L),
    the triangle (L r0, L r1, L r2) has its normal pointing away from L iff d > 0; it is kept if that is the outside (L inside),
    else its last two vertices are swapped;
  * two inside A < B, two outside C < D: with d = det(B - A, C - A, D - A) the quad cycle (AC, AD, BD, BC) is outward iff
    d > 0, else (AC, BC, BD, AD) is; triangles (q0, q1, q2), (q0, q2, q3): the diagonal is always AC - BD.
"""
import itertools

import numpy as np

PERMUTATIONS = tuple(itertools.permutations(range(3)))          # tetrahedron q <-> the q-th permutation, lexicographic


def tet_vertices(q):
    """The four corner offsets (dx, dy, dz) of tetrahedron q: c, c + e_a, c + e_a + e_b, c + (1, 1, 1)."""
    v, out = [0, 0, 0], [(0, 0, 0)]
    for axis in PERMUTATIONS[q]:
        v[axis] = 1
        out.append(tuple(v))
    return out


def _det(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def case_triangles(q, s):
    """Triangles of tetrahedron q in sign case s (bit m: vertex m inside) as triples of (m, n) vertex-number pairs, m < n."""
    pos = tet_vertices(q)
    inside = [m for m in range(4) if (s >> m) & 1]
    outside = [m for m in range(4) if not (s >> m) & 1]
    pair = lambda m, n: (min(m, n), max(m, n))
    if len(inside) in (0, 4):
        return []
    if len(inside) == 2:
        (a, b), (c, d) = inside, outside
        det = _det(_sub(pos[b], pos[a]), _sub(pos[c], pos[a]), _sub(pos[d], pos[a]))
        cyc = [pair(a, c), pair(a, d), pair(b, d), pair(b, c)] if det > 0 else [pair(a, c), pair(b, c), pair(b, d), pair(a, d)]
        return [(cyc[0], cyc[1], cyc[2]), (cyc[0], cyc[2], cyc[3])]
    lone, rest, lone_inside = (inside[0], outside, True) if len(inside) == 1 else (outside[0], inside, False)
    det = _det(*[_sub(pos[r], pos[lone]) for r in rest])
    tri = [pair(lone, r) for r in rest]
    if (det > 0) != lone_inside:
        tri = [tri[0], tri[2], tri[1]]
    return [tuple(tri)]


def grid_coords(origin, step, shape):
    """fp32(origin + idx * step) per axis: the float64 product and sum, rounded once."""
    return [(np.float64(origin[a]) + np.arange(shape[a], dtype=np.float64) * np.float64(step[a])).astype(np.float32)
            for a in range(3)]


def isosurface_reference(field, level, origin, step):
    """-> vertices [V,3] float32, faces [T,3] int32, cases [6,16] int64 (cells per tetrahedron and sign case)."""
    f = np.ascontiguousarray(field, dtype=np.float32)
    nx, ny, nz = shape = f.shape
    level = np.float32(level)
    with np.errstate(invalid="ignore"):
        inside = f > level                                      # NaN is not inside
    ids = np.arange(f.size, dtype=np.int64).reshape(shape)
    xs = grid_coords(origin, step, shape)
    cases = np.zeros((6, 16), dtype=np.int64)
    if min(shape) < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), cases

    def sl(off, far):
        """Slices of the points p with p + far in the grid, shifted by `off`."""
        return tuple(slice(off[a], shape[a] - far[a] + off[a]) for a in range(3))

    # ---- vertices: one per crossed edge (p, p + e), ordered by (p, type = 4 ex + 2 ey + ez)
    keys, va, vb, ia, es = [], [], [], [], []
    for t in range(1, 8):
        e = ((t >> 2) & 1, (t >> 1) & 1, t & 1)
        a, b = sl((0, 0, 0), e), sl(e, e)
        crossed = inside[a] != inside[b]
        keys.append(ids[a][crossed] * 7 + (t - 1))
        va.append(f[a][crossed])
        vb.append(f[b][crossed])
        ia.append(ids[a][crossed])
        es.append(np.broadcast_to(np.array(e, dtype=np.int64), (int(crossed.sum()), 3)))
    keys, va, vb, ia, es = (np.concatenate(x) for x in (keys, va, vb, ia, es))
    order = np.argsort(keys, kind="stable")
    keys, va, vb, ia, es = keys[order], va[order], vb[order], ia[order], es[order]
    idx = np.stack(np.unravel_index(ia, shape), axis=1) if len(ia) else np.zeros((0, 3), np.int64)
    with np.errstate(all="ignore"):
        tau = (level - va) / (vb - va)                            # float32 throughout, one rounding per operation
        vertices = np.empty((len(keys), 3), dtype=np.float32)
        for a in range(3):
            xa = xs[a][idx[:, a]]
            xb = xs[a][np.minimum(idx[:, a] + es[:, a], shape[a] - 1)]
            vertices[:, a] = xa + tau * (xb - xa)
    assert vertices.dtype == np.float32 and tau.dtype == np.float32

    # ---- triangles: per cell, tetrahedron 0..5, triangle 0..1
    far = (1, 1, 1)
    cell_ids = ids[sl((0, 0, 0), far)]
    rows = []                                                    # (cell, q, triangle, three edge keys)
    for q in range(6):
        verts = tet_vertices(q)
        s = np.zeros(cell_ids.shape, dtype=np.int64)
        for m, v in enumerate(verts):
            s |= inside[sl(v, far)].astype(np.int64) << m
        cases[q] = np.bincount(s.ravel(), minlength=16)
        for case in range(1, 15):
            cells = cell_ids[s == case]
            if not len(cells):
                continue
            for k, tri in enumerate(case_triangles(q, case)):
                ek = []
                for m, n in tri:
                    lo, hi = verts[m], verts[n]                  # lo <= hi componentwise: the owner is cell + lo
                    owner = cells + (lo[0] * ny + lo[1]) * nz + lo[2]
                    t = 4 * (hi[0] - lo[0]) + 2 * (hi[1] - lo[1]) + (hi[2] - lo[2])
                    ek.append(owner * 7 + (t - 1))
                rows.append(np.stack([cells, np.full_like(cells, q), np.full_like(cells, k)] + ek, axis=1))
    if not rows:
        return vertices, np.zeros((0, 3), np.int32), cases
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    vid = np.searchsorted(keys, rows[:, 3:])
    assert (keys[vid] == rows[:, 3:]).all()                      # every triangle corner is a crossed edge
    return vertices, vid.astype(np.int32), cases


# ---- analytic fields (inside = f > level), on the box [-1, 1]^3 ---------------------------------------------------------------
BOX_ORIGIN = (-1.0, -1.0, -1.0)


def box_step(shape):
    return tuple(2.0 / (n - 1) if n > 1 else 0.0 for n in shape)


SPHERE_R = 0.6
LEVELS = {"sphere": 0.0, "two_spheres": 0.0, "torus": 0.0, "sinusoids": 0.1, "random": 0.5}


def analytic_field(name, shape, seed=0):
    """float32 [nx,ny,nz]; float64 arithmetic, rounded once (the same array goes to the kernel and to the restatement)."""
    if name == "random":
        return np.random.default_rng(seed).random(shape, dtype=np.float32)
    step = box_step(shape)
    x, y, z = np.meshgrid(*[BOX_ORIGIN[a] + np.arange(shape[a], dtype=np.float64) * step[a] for a in range(3)], indexing="ij")
    if name == "sphere":
        f = SPHERE_R - np.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.05) ** 2)
    elif name == "two_spheres":
        f = np.maximum(0.3 - np.sqrt((x + 0.45) ** 2 + (y - 0.02) ** 2 + (z - 0.03) ** 2),
                       0.3 - np.sqrt((x - 0.45) ** 2 + (y + 0.04) ** 2 + (z - 0.01) ** 2))
    elif name == "torus":
        f = 0.2 - np.sqrt((np.sqrt((x - 0.01) ** 2 + (y + 0.02) ** 2) - 0.55) ** 2 + (z - 0.03) ** 2)
    elif name == "sinusoids":
        f = np.sin(3 * x + 0.3) + np.sin(4 * y + 0.5) * np.cos(2 * z) + 0.5 * np.sin(5 * x * z - 0.2)
    else:
        raise KeyError(name)
    return f.astype(np.float32)


# ---- mesh measures ----------------------------------------------------------------------------------------------------------------
def mesh_stats(vertices, faces):
    """Topology and size of an indexed triangle mesh (float64)."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(faces, dtype=np.int64)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    dkey = directed[:, 0] * (len(v) + 1) + directed[:, 1]
    und = np.sort(directed, axis=1)
    _, ucount = np.unique(und[:, 0] * (len(v) + 1) + und[:, 1], return_counts=True)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cross = np.cross(p1 - p0, p2 - p0)
    return {
        "V": len(v), "T": len(t), "E": len(ucount),
        "euler": len(v) - len(ucount) + len(t),
        "closed": bool((ucount == 2).all()),                     # every undirected edge lies in exactly two faces
        "oriented": len(np.unique(dkey)) == len(dkey),           # every directed edge occurs once
        "used_all_vertices": len(np.unique(t)) == len(v),
        "area": float(0.5 * np.sqrt((cross ** 2).sum(1)).sum()),
        "volume": float((p0 * cross).sum() / 6.0),               # signed: positive for outward normals
    }
