"""CPU checks of the mesh clean-up: the NumPy restatement tests/mesh_components_reference.py on hand-made
meshes with known answers, write_ply_colors against an independent reader, argument errors before any library call, and the
new names in the package's and the library's export lists."""
import struct

import numpy as np
import pytest
import torch

import mesh_components_reference as M


def _tetra(base):
    """The four faces of a tetrahedron on the vertices base..base+3."""
    a, b, c, d = range(base, base + 4)
    return [[a, b, c], [a, c, d], [a, d, b], [b, d, c]]


def test_restatement_on_hand_made_meshes():
    # two tetrahedra (vertices 1..4 and 6..9), the isolated vertices 0, 5 and 10, a duplicate and a degenerate face
    faces = np.array(_tetra(6) + _tetra(1) + [[6, 7, 8]] + [[9, 9, 8]])
    vl, fl, (cl, cf, cv) = M.components_reference(faces, 11)
    assert vl.tolist() == [0, 1, 1, 1, 1, 5, 6, 6, 6, 6, 10]
    assert fl.tolist() == [6] * 4 + [1] * 4 + [6, 6]
    assert cl.tolist() == [0, 1, 5, 6, 10] and cf.tolist() == [0, 4, 0, 6, 0] and cv.tolist() == [1, 4, 1, 4, 1]
    assert all(a.dtype == np.int32 for a in (vl, fl, cl, cf, cv))
    # a face that names V or -1 joins nothing and has the label -1; the rest is labelled as without it
    bad = np.concatenate([faces, [[0, 5, 11]], [[-1, 5, 10]]])
    vl2, fl2, table2 = M.components_reference(bad, 11)
    assert np.array_equal(vl2, vl) and fl2.tolist() == fl.tolist() + [-1, -1]
    assert all(np.array_equal(a, b) for a, b in zip(table2, (cl, cf, cv)))
    # no faces, no vertices
    vl, fl, (cl, cf, cv) = M.components_reference(np.zeros((0, 3), int), 5)
    assert vl.tolist() == [0, 1, 2, 3, 4] and len(fl) == 0 and cl.tolist() == [0, 1, 2, 3, 4] and cf.tolist() == [0] * 5 and cv.tolist() == [1] * 5
    vl, fl, (cl, cf, cv) = M.components_reference(np.zeros((0, 3), int), 0)
    assert len(vl) == len(fl) == len(cl) == len(cf) == len(cv) == 0
    vl, fl, (cl, _, _) = M.components_reference(np.array([[0, 0, 0]]), 0)
    assert len(vl) == 0 and fl.tolist() == [-1] and len(cl) == 0


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_restatement_on_a_strip(order):
    """A triangle strip is one chain: every label is the smallest id, whatever the numbering; two interleaved strips are two."""
    n = 257
    ids = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": np.random.default_rng(3).permutation(n)}[order]
    strip = np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1)
    vl, fl, (cl, cf, cv) = M.components_reference(strip, n)
    assert (vl == 0).all() and (fl == 0).all() and cl.tolist() == [0] and cf.tolist() == [n - 2] and cv.tolist() == [n]
    two = np.concatenate([2 * strip[:100], 2 * strip[:100] + 1])
    vl, fl, (cl, cf, cv) = M.components_reference(two, 2 * n)
    used, lo = np.unique(two), 2 * int(strip[:100].min())              # the chains' smallest ids: lo and lo + 1
    assert np.array_equal(vl[used], lo + used % 2) and fl.tolist() == [lo] * 100 + [lo + 1] * 100
    big = np.isin(cl, [lo, lo + 1])
    assert big.sum() == 2 and cf[big].tolist() == [100, 100] and cv[big].tolist() == [102, 102]
    assert (cf[~big] == 0).all() and (cv[~big] == 1).all() and len(cl) == 2 * n - 204 + 2


def test_restatement_filter_keeps_order_and_breaks_ties_by_label():
    # components: {6..9} with 5 faces, {1..4} with 4, {10,11,12} with 1, {13,14,15} with 1; 0 and 5 isolated
    faces = np.array(_tetra(6)[:2] + [[10, 11, 12]] + _tetra(1) + _tetra(6)[2:] + [[15, 14, 13]] + [[6, 7, 8]])
    v = np.arange(16 * 3, dtype=np.float32).reshape(16, 3)
    table = M.components_reference(faces, 16)[2]
    assert table[0].tolist() == [0, 1, 5, 6, 10, 13] and table[1].tolist() == [0, 4, 0, 5, 1, 1]
    assert M.select_reference(table, keep_largest=1) == {6} and M.select_reference(table, keep_largest=3) == {6, 1, 10}
    assert M.select_reference(table, keep_largest=4) == {6, 1, 10, 13} and M.select_reference(table, keep_largest=5) == {6, 1, 10, 13, 0}
    assert M.select_reference(table, min_triangles=4) == {1, 6} and M.select_reference(table, min_triangles=5) == {6}
    assert M.select_reference(table, min_triangles=1, keep_largest=5) == {1, 6, 10, 13}
    assert M.select_reference(table, min_triangles=5, keep_largest=0) == set()
    fv, ff, idx = M.filter_reference(v, faces, keep_largest=3)
    assert idx.tolist() == [1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12] and np.array_equal(fv, v[idx])
    kept_faces = faces[[0, 1, 2, 3, 4, 5, 6, 7, 8, 10]]               # all but the face of {13,14,15}, order kept
    assert np.array_equal(idx[ff], kept_faces) and ff.dtype == np.int32
    fv, ff, idx = M.filter_reference(v, faces, min_triangles=6)
    assert fv.shape == (0, 3) and ff.shape == (0, 3) and idx.shape == (0,)
    fv, ff, idx = M.filter_reference(v, faces, keep_largest=99)        # the identity
    assert np.array_equal(fv, v) and np.array_equal(ff, faces) and idx.tolist() == list(range(16))


# ---- write_ply ------------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    """An independent reader: the header's property lists decide the layout.  -> dict of per-vertex columns, faces [T,3]."""
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[-1] == ""
    sizes = {"float": ("f", 4), "uchar": ("B", 1), "int": ("i", 4)}
    elements = []
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        else:
            assert w[0] == "property"
            elements[-1][2].append(tuple(w[1:]))
    assert [e[0] for e in elements] == ["vertex", "face"] and elements[1][2] == [("list", "uchar", "int", "vertex_indices")]
    _, n_v, props = elements[0]
    fmt = "<" + "".join(sizes[t][0] for t, _ in props)
    row = struct.calcsize(fmt)
    assert row == sum(sizes[t][1] for t, _ in props) and len(body) == row * n_v + 13 * elements[1][1]
    cols = {name: [] for _, name in props}
    for k in range(n_v):
        for (_, name), x in zip(props, struct.unpack_from(fmt, body, row * k)):
            cols[name].append(x)
    faces = []
    for k in range(elements[1][1]):
        n, a, b, c = struct.unpack_from("<Biii", body, row * n_v + 13 * k)
        assert n == 3
        faces.append([a, b, c])
    return [name for _, name in props], cols, np.array(faces, dtype=np.int32).reshape(-1, 3)


V3 = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, -2.0]])
F3 = torch.tensor([[0, 1, 2]], dtype=torch.int32)
# what write_ply wrote for (V3, F3) before it knew colours
PLAIN_BYTES = (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
               b"element face 1\nproperty list uchar int vertex_indices\nend_header\n"
               b"\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x80?\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\xc0?"
               b"\x00\x00\x00\xc0\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00")


def test_write_ply_without_colours_is_unchanged(tmp_path):
    from nerf_replication_amd.mesh import write_ply, write_ply_colors
    path = str(tmp_path / "plain.ply")
    write_ply(path, V3, F3)
    assert open(path, "rb").read() == PLAIN_BYTES
    write_ply_colors(path, V3, F3, None, None)
    assert open(path, "rb").read() == PLAIN_BYTES
    write_ply_colors(path, V3, F3, colors=None)
    assert open(path, "rb").read() == PLAIN_BYTES


def test_write_ply_with_colours(tmp_path):
    from nerf_replication_amd.mesh import write_ply_colors as write_ply
    rng = np.random.default_rng(11)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    nrm = rng.standard_normal((7, 3)).astype(np.float32)
    col = rng.random((7, 3)).astype(np.float32)
    # the rounding's corners: below 0, above 1, the half-way points k + 0.5 over 255 (floor(x + 0.5) rounds them up), NaN
    col[0] = [-0.25, 1.75, 0.0]
    col[1] = [1.0, np.float32(0.5 / 255), np.float32(254.5 / 255)]
    col[2] = [np.float32(127.5 / 255), np.nextafter(np.float32(127.5 / 255), np.float32(0)), np.nan]
    want = np.floor(np.clip(np.nan_to_num(col.astype(np.float64), nan=0.0), 0, 1) * 255 + 0.5).astype(np.int64)
    assert want[0].tolist() == [0, 255, 0] and want[1, 0] == 255 and want[2, 2] == 0
    path = str(tmp_path / "c.ply")

    write_ply(path, torch.from_numpy(v), torch.from_numpy(f), colors=torch.from_numpy(col))
    names, cols, faces = _read_ply(path)
    assert names == ["x", "y", "z", "red", "green", "blue"]
    assert np.array_equal(np.array([cols[n] for n in "xyz"], dtype=np.float32).T.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(np.array([cols[n] for n in ("red", "green", "blue")]).T, want) and np.array_equal(faces, f)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii")
    assert head == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 5\n"
                    "property list uchar int vertex_indices\n")

    write_ply(path, v, f, normals=nrm, colors=col)                      # arrays are taken as tensors are
    names, cols, faces = _read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.array([cols[n] for n in "xyz"], dtype=np.float32).T.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(np.array([cols[n] for n in ("nx", "ny", "nz")], dtype=np.float32).T.view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(np.array([cols[n] for n in ("red", "green", "blue")]).T, want) and np.array_equal(faces, f)
    body = open(path, "rb").read().split(b"end_header\n", 1)[1]
    assert len(body) == 27 * 7 + 13 * 5 and body[24:27] == bytes(want[0].tolist())      # 6 floats, then 3 bytes: no padding

    write_ply(path, v, f, normals=nrm)                                  # normals alone: as before
    names, cols, _ = _read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz"]
    with pytest.raises(ValueError):
        write_ply(path, v, f, colors=col[:6])
    with pytest.raises(ValueError):
        write_ply(path, v, f, colors=np.zeros((7, 4), np.float32))


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_library_call(tmp_path, monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import mesh
    monkeypatch.setattr(pkg._lib, "load", lambda: pytest.fail("argument errors must not reach the library"))
    v, f = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError):
        mesh.filter_components(v, f)                                    # neither criterion
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            mesh.filter_components(v, f, min_triangles=bad)
        with pytest.raises(ValueError):
            mesh.filter_components(v, f, keep_largest=bad)
    for bad_v, bad_f in ((torch.zeros(4, 2), f), (v, torch.zeros((2, 4), dtype=torch.int32)), (v, torch.zeros(2, 3)),
                         (torch.zeros((4, 3), dtype=torch.int32), f), (v.numpy(), f), (v, f.numpy())):
        with pytest.raises(ValueError):
            mesh.filter_components(bad_v, bad_f, keep_largest=1)
    with pytest.raises(ValueError):
        mesh.mesh_components(torch.zeros(2, 3), 4)
    for bad_n in (-1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError):
            mesh.mesh_components(f, bad_n)

    net = pkg.Network()                                                 # on the CPU: a GPU call would raise NerfLibraryError instead
    out = str(tmp_path / "m.ply")
    box = [-1, -1, -1, 1, 1, 1]
    with pytest.raises(TypeError):
        mesh.extract_mesh(lambda x: x, 1.0, box, out, 8, colors=True)   # colours need the network
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            mesh.extract_mesh(net, 1.0, box, out, 8, min_triangles=bad)
        with pytest.raises(ValueError):
            mesh.extract_mesh(net, 1.0, box, out, 8, keep_largest=bad)
    with pytest.raises(TypeError):
        mesh.vertex_colors(lambda x: x, v)
    with pytest.raises(ValueError):
        mesh.vertex_colors(net, v, model="medium")
    with pytest.raises(ValueError):
        mesh.vertex_colors(net, torch.zeros(4, 2))
    with pytest.raises(ValueError):
        mesh.vertex_colors(net, v, viewdirs=torch.zeros(3, 3))
    import os
    assert not os.path.exists(out)


def test_the_new_names_are_exported():
    import nerf_replication_amd as pkg
    for name in ("mesh_components", "filter_components", "vertex_colors", "write_ply_colors"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)) and name in dir(pkg)
    for name in ("nerf_mesh_components_workspace_bytes", "nerf_mesh_components", "nerf_mesh_filter_count", "nerf_mesh_filter_emit"):
        assert name in pkg._lib.EXPORTS


def test_size_entries_refuse_without_a_gpu():
    """More than 2^31 - 1 vertices or faces: refused by the size check, which touches neither a pointer nor the device."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    big = 2 ** 31
    assert lib.nerf_mesh_components_workspace_bytes(big, 1) == -1 and lib.nerf_mesh_components_workspace_bytes(1, big) == -1
    assert lib.nerf_mesh_components_workspace_bytes(-1, 1) == -1
    assert lib.nerf_mesh_components_workspace_bytes(0, 0) == 0
    # components: three int32 per vertex and one per 256 vertices; filter: one per vertex and face, one per 256 of each
    assert lib.nerf_mesh_components_workspace_bytes(1000, 10) == 3 * 4096 + 256
    assert lib.nerf_mesh_components_workspace_bytes(1000, 5000) == 4096 + 20224 + 256 + 256
    for v, t in ((big, 1), (1, big)):
        assert lib.nerf_mesh_components(None, t, v, None, None, None, None, None, None, None, None) == -1
        assert b"2^31" in lib.nerf_last_error()
        assert lib.nerf_mesh_filter_count(None, None, None, v, t, None, None, None) == -1
        assert lib.nerf_mesh_filter_emit(None, None, v, t, None, None, None, None, None) == -1
    assert lib.nerf_mesh_components(None, 0, 5, None, None, None, None, None, None, None, None) == -1      # null n_components
