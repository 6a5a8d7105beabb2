"""CPU checks of the iso-surface feature (nerf_replication_amd/mesh.py): the NumPy restatement
tests/isosurface_reference.py against analytic fields, the committed case table against its generator and against the
restatement's own enumeration, the PLY writer, and extract_mesh's argument checks.  The kernels themselves are compared with the
restatement in tests/test_gpu_mesh.py."""
import importlib.util
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import isosurface_reference as R
from conftest import REPO


def _mesh(name, n):
    shape = (n, n, n)
    v, f, cases = R.isosurface_reference(R.analytic_field(name, shape), R.LEVELS[name], R.BOX_ORIGIN, R.box_step(shape))
    return v, f, cases


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("two_spheres", 4), ("torus", 0)])
@pytest.mark.parametrize("n", [24, 33])
def test_restatement_gives_closed_oriented_manifolds(name, euler, n):
    """Level sets strictly inside the grid: every undirected edge lies in exactly two faces, every directed edge occurs once,
    the Euler characteristic is that of the surface, the signed volume is positive (normals point out of the blob)."""
    v, f, _ = _mesh(name, n)
    st = R.mesh_stats(v, f)
    assert st["T"] > 0 and st["closed"] and st["oriented"] and st["used_all_vertices"]
    assert st["euler"] == euler
    assert st["volume"] > 0
    assert np.isfinite(v).all() and np.abs(v).max() < 1.0


@pytest.mark.parametrize("n", [24, 48])
def test_restatement_sphere_area_and_volume(n):
    """The mesh is inscribed (its vertices lie on the sphere up to the linear interpolation of a distance field), so area and
    volume fall short by O((h / r)^2), h the grid step.  Margin: (h / r)^2.  Measured relative errors:
        n = 24: area -5.42e-3, volume -1.05e-2   (margin 2.10e-2)
        n = 48: area -1.29e-3, volume -2.52e-3   (margin 5.03e-3)
    i.e. the volume error is half the margin at both resolutions and quarters when h halves."""
    v, f, _ = _mesh("sphere", n)
    st = R.mesh_stats(v, f)
    r, h = R.SPHERE_R, 2.0 / (n - 1)
    margin = (h / r) ** 2
    area_err = st["area"] / (4 * math.pi * r * r) - 1
    vol_err = st["volume"] / (4 / 3 * math.pi * r ** 3) - 1
    print(f"n={n}: area {area_err:+.3e} volume {vol_err:+.3e} margin {margin:.3e}")
    assert -margin <= area_err <= 0 and -margin <= vol_err <= 0


def test_restatement_random_field_exercises_every_case():
    """rand at level 0.5: all 16 sign cases occur in all six tetrahedra; the mesh is open at the boundary, every index valid."""
    f = R.analytic_field("random", (12, 11, 13))
    v, t, cases = R.isosurface_reference(f, R.LEVELS["random"], R.BOX_ORIGIN, R.box_step(f.shape))
    assert cases.shape == (6, 16) and (cases > 0).all()
    assert (cases.sum(1) == 11 * 10 * 12).all()
    assert len(t) == int(sum(cases[q, s] * len(R.case_triangles(q, s)) for q in range(6) for s in range(16)))
    assert t.min() >= 0 and t.max() < len(v) and len(np.unique(t)) == len(v)
    assert R.mesh_stats(v, t)["oriented"]


def test_restatement_degenerate_inputs():
    z = np.zeros((0, 3))
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        v, t, _ = R.isosurface_reference(R.analytic_field("random", shape), 0.5, R.BOX_ORIGIN, R.box_step(shape))
        assert v.shape == z.shape and t.shape == z.shape
    f = R.analytic_field("sphere", (9, 9, 9))
    for level in (-10.0, 10.0):                                   # all inside / no crossing
        v, t, _ = R.isosurface_reference(f, level, R.BOX_ORIGIN, R.box_step(f.shape))
        assert len(v) == 0 and len(t) == 0
    # a value equal to the level is outside; NaN is outside
    g = np.full((3, 3, 3), 1.0, np.float32)
    g[1, 1, 1] = 0.0
    v, t, _ = R.isosurface_reference(g, 0.0, R.BOX_ORIGIN, R.box_step(g.shape))
    st = R.mesh_stats(v, t)
    assert st["V"] == 14 and st["closed"] and st["euler"] == 2      # a (collapsed) hole around the centre point
    assert (v == 0).all(axis=1).sum() == 14                        # tau lands on the centre point exactly
    g[1, 1, 1] = np.nan
    v2, t2, _ = R.isosurface_reference(g, 0.0, R.BOX_ORIGIN, R.box_step(g.shape))
    assert np.array_equal(t, t2) and np.isnan(v2).all()


def _generator():
    spec = importlib.util.spec_from_file_location("gen_isosurface_table", os.path.join(REPO, "tools", "gen_isosurface_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_case_table_is_what_the_generator_writes():
    gen = _generator()
    assert open(gen.OUT).read() == gen.render()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_isosurface_table.py"), "--check"])
    assert r.returncode == 0


def test_case_table_agrees_with_the_restatement():
    """Two derivations of the winding (the generator: midpoint geometry; the restatement: the tetrahedron's signed volume) and of
    the quad split give the same 96 cases."""
    gen = _generator()
    tets, ntri, refs, cube = gen.build()
    for q, codes in enumerate(tets):
        assert [4 * v[0] + 2 * v[1] + v[2] for v in R.tet_vertices(q)] == codes
        for s in range(16):
            mine = [gen.edge_byte(codes[m], codes[n]) for tri in R.case_triangles(q, s) for m, n in tri]
            assert ntri[q][s] * 3 == len(mine) and refs[q][s][:len(mine)] == mine, (q, s)
    assert cube[0] == cube[255] == 0 and max(cube) == 12


def test_write_ply_round_trip(tmp_path):
    from nerf_replication_amd.mesh import write_ply
    v, f, _ = _mesh("sphere", 9)
    path = str(tmp_path / "sphere.ply")
    write_ply(path, torch.from_numpy(v), torch.from_numpy(f))
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n") == [
        "ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
        "property float z", f"element face {len(f)}", "property list uchar int vertex_indices", ""]
    assert len(body) == 12 * len(v) + 13 * len(f)
    assert body[:12 * len(v)] == v.astype("<f4").tobytes()
    for k in (0, len(f) // 2, len(f) - 1):
        n, a, b, c = struct.unpack_from("<Biii", body, 12 * len(v) + 13 * k)
        assert n == 3 and [a, b, c] == f[k].tolist()
    faces = np.frombuffer(body[12 * len(v):], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert (faces["n"] == 3).all() and np.array_equal(faces["i"], f)
    with pytest.raises(ValueError):
        write_ply(path, torch.zeros(4, 2), torch.zeros(1, 3, dtype=torch.int32))


def test_extract_mesh_argument_errors_come_before_any_gpu_call(tmp_path, monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import mesh
    monkeypatch.setattr(pkg._lib, "load", lambda: pytest.fail("argument errors must not reach the library"))
    net = pkg.Network()                                           # on the CPU: a GPU call would raise NerfLibraryError instead
    out = str(tmp_path / "m.ply")
    box = [-1, -1, -1, 1, 1, 1]
    with pytest.raises(TypeError):
        mesh.extract_mesh(3.0, 1.0, box, out, 8)
    with pytest.raises(ValueError):
        mesh.extract_mesh(net, 1.0, None, out, 8)
    for bad_box in ([0, 0, 0, 1, 1], [0, 0, 0, 1, 1, float("nan")], [0, 0, 0, 1, 1, -1], "box"):
        with pytest.raises(ValueError):
            mesh.extract_mesh(net, 1.0, bad_box, out, 8)
    for bad_n in (0, -3, (4, 4), (4, 0, 4), 2.5, (2048, 2048, 512), "8"):
        with pytest.raises(ValueError):
            mesh.extract_mesh(net, 1.0, box, out, bad_n)
    for bad_level in ("high", float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mesh.extract_mesh(net, bad_level, box, out, 8)
    with pytest.raises(TypeError):
        mesh.extract_mesh(net, 1.0, box, 17, 8)
    with pytest.raises(ValueError):
        mesh.density_grid(net, box, 8, model="medium")
    with pytest.raises(ValueError):
        mesh.density_grid(net, box, 8, chunk_lines=0)
    assert not os.path.exists(out)


def test_extract_mesh_defaults_and_grid_axes():
    from nerf_replication_amd import mesh
    assert (mesh.DEFAULT_LEVEL, mesh.DEFAULT_RESOLUTION) == (32.0, 256)       # cfg.level / cfg.resolution of the reference
    axes, origin, step = mesh.grid_axes([-1, 0, 2, 1, 3, 2], (5, 4, 1))
    assert [len(a) for a in axes] == [5, 4, 1] and origin == (-1.0, 0.0, 2.0) and step == (0.5, 1.0, 0.0)
    assert axes[0][-1] == 1.0 and axes[1][-1] == 3.0 and axes[2][0] == 2.0


def test_size_entries_refuse_without_a_gpu():
    """The size checks of the three entries come first and touch neither a pointer nor the device."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    assert lib.nerf_isosurface_workspace_bytes(2048, 2048, 512) == -1                  # 2^31 points
    assert lib.nerf_isosurface_workspace_bytes(4, -1, 4) == -1
    assert lib.nerf_isosurface_workspace_bytes(33, 33, 33) == (4 * 33 ** 3 + 255) // 256 * 256 + 2 * 768   # 141 blocks
    assert lib.nerf_isosurface_workspace_bytes(0, 5, 5) == 0 and lib.nerf_isosurface_workspace_bytes(1, 1, 1) == 256 + 2 * 256
    assert lib.nerf_isosurface_count(None, 1, 2048, 2048, 512, 0.0, None, None, None) == -1
    assert b"2^31" in lib.nerf_last_error()
    assert lib.nerf_isosurface_emit(None, 1, 2048, 2048, 512, 0.0, None, None, None, None, None, None) == -1
    assert lib.nerf_isosurface_count(None, 0, 4, 4, 4, 0.0, None, None, None) == -1    # stride < 1
    assert lib.nerf_isosurface_count(None, 1, 4, 4, 4, 0.0, None, None, None) == -1    # null counts
    assert lib.nerf_isosurface_emit(None, 1, 4, 1, 4, 0.0, None, None, None, None, None, None) == 0     # no cells: a no-op
