"""GPU tests of the mesh clean-up: nerf_mesh_components and nerf_mesh_filter_* against the NumPy restatement
tests/mesh_components_reference.py (every array exactly, vertices bit for bit), hand-made index lists at the sizes where a union-find
goes wrong, vertex_colors against the CPU oracle, and extract_mesh with the filter, normals and colours end to end.  The meshes are
those of the restatement isosurface_reference on the analytic fields of test_gpu_mesh.py (its cached cases are shared)."""
import functools
import struct

import numpy as np
import pytest
import torch

import isosurface_reference as R
import mesh_components_reference as M
from gpu_common import amd, network  # noqa: F401
from test_gpu_mesh import FIELDS, SHAPES, _bits, _case

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -77, 5
WS_PAD = 512                       # bytes of sentinel on both sides of the workspace
WS_BYTE = 0xA5


@functools.lru_cache(maxsize=None)
def _components(name, shape):
    _, v, t = _case(name, shape)
    out = M.components_reference(t, len(v))
    for a in (out[0], out[1]) + out[2]:
        a.setflags(write=False)
    return out


def _padded(n, dtype=torch.int32, fill=SENTINEL):
    """A buffer of n elements as the interior of a larger sentinel-filled one -> (whole, interior)."""
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n]


def _intact(whole, n, fill=SENTINEL):
    return bool((whole[:PAD] == fill).all() and (whole[PAD + n:] == fill).all())


def _run_components(amd, faces, V):
    """nerf_mesh_components through the C ABI.  faces: numpy [T,3].  The label buffers and the workspace (which holds parent[]) are
    interior slices of sentinel-filled tensors, the table has PAD spare rows -> dict of device tensors; the sentinels are checked."""
    L = amd._lib
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).cuda()
    T = f.shape[0]
    nbytes = int(L.call("nerf_mesh_components_workspace_bytes", V, T))
    assert nbytes >= 0
    ws_whole = torch.full((nbytes + 2 * WS_PAD,), WS_BYTE, dtype=torch.uint8, device="cuda")
    ws = ws_whole[WS_PAD:WS_PAD + nbytes]
    vl_whole, vl = _padded(V)
    fl_whole, fl = _padded(T)
    table = torch.full((3, V + PAD), SENTINEL, dtype=torch.int32, device="cuda")
    n_comp = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    L.call("nerf_mesh_components", f, T, V, ws, vl, fl, table[0], table[1], table[2], n_comp)
    torch.cuda.synchronize()
    C = int(n_comp.item())
    assert 0 <= C <= V
    assert _intact(vl_whole, V) and _intact(fl_whole, T)
    assert bool((ws_whole[:WS_PAD] == WS_BYTE).all() and (ws_whole[WS_PAD + nbytes:] == WS_BYTE).all())
    assert bool((table[:, C:] == SENTINEL).all())                              # the rows past the count are untouched
    return {"faces": f, "V": V, "T": T, "C": C, "vertex_label": vl, "face_label": fl, "table": table, "workspace": ws,
            "whole": (vl_whole, fl_whole)}


def _assert_components(out, ref):
    ref_vl, ref_fl, ref_table = ref
    assert out["C"] == len(ref_table[0])
    assert np.array_equal(out["vertex_label"].cpu().numpy(), ref_vl)
    assert np.array_equal(out["face_label"].cpu().numpy(), ref_fl)
    for row, want in zip(out["table"], ref_table):
        assert np.array_equal(row[:out["C"]].cpu().numpy(), want)


# ---- 1. labels equal the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", FIELDS)
def test_components_equal_the_restatement(amd, name, shape):
    _, v, t = _case(name, shape)
    ref = _components(name, shape)
    if name == "two_spheres" and len(t):
        assert len(ref[2][0]) == 2
    if name == "sinusoids":
        assert len(ref[2][0]) == (2 if shape == (2, 2, 2) else 5)
    if name == "random" and shape != (2, 2, 2):
        assert len(ref[2][0]) == {(9, 12, 17): 6, (33, 33, 33): 17, (67, 63, 66): 57}[shape]
    out = _run_components(amd, t, len(v))
    _assert_components(out, ref)
    again = _run_components(amd, t, len(v))                                     # atomics with a unique result: the same bytes
    assert torch.equal(again["whole"][0], out["whole"][0]) and torch.equal(again["whole"][1], out["whole"][1])
    assert torch.equal(again["table"], out["table"])
    vl, fl, table = amd.mesh_components(out["faces"], len(v))                   # the Python interface
    assert vl.dtype == fl.dtype == torch.int32 and vl.shape == (len(v),) and fl.shape == (len(t),)
    assert torch.equal(vl, out["vertex_label"]) and torch.equal(fl, out["face_label"])
    assert all(r.dtype == torch.int32 and torch.equal(r, row[:out["C"]]) for r, row in zip(table, out["table"]))
    assert table._fields == ("label", "faces", "vertices")


# ---- 2. hand-made index lists ------------------------------------------------------------------------------------------------------
def _strip(ids):
    return np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1)


def _numbering(order, n):
    return {"ascending": np.arange(n), "descending": np.arange(n)[::-1].copy(),
            "permuted": np.random.default_rng(1000 + n).permutation(n)}[order]


def test_components_without_faces_or_vertices(amd):
    out = _run_components(amd, np.zeros((0, 3), np.int32), 5)                   # every vertex on its own
    assert out["C"] == 5 and out["vertex_label"].tolist() == [0, 1, 2, 3, 4]
    assert out["table"][:, :5].tolist() == [[0, 1, 2, 3, 4], [0] * 5, [1] * 5]
    out = _run_components(amd, np.zeros((0, 3), np.int32), 0)
    assert out["C"] == 0
    out = _run_components(amd, np.array([[0, 1, 2], [0, 0, 0]]), 0)             # no vertex: every index is out of range
    assert out["C"] == 0 and out["face_label"].tolist() == [-1, -1]
    vl, fl, table = amd.mesh_components(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 0)
    assert vl.shape == (0,) and fl.shape == (0,) and all(r.shape == (0,) for r in table)
    v2, f2, idx = amd.filter_components(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), keep_largest=1)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and idx.shape == (0,)
    v2, f2, idx = amd.filter_components(torch.ones((5, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), keep_largest=2)
    assert v2.shape == (2, 3) and f2.shape == (0, 3) and idx.tolist() == [0, 1]  # five components of no faces: the two lowest labels


def test_components_isolated_duplicate_and_degenerate(amd):
    # vertices 0, 5 and 10 are named by no face; [6,7,8] comes twice; [9,9,8] is degenerate and is what ties 9 to the rest
    faces = np.array([[6, 7, 8], [1, 2, 3], [3, 2, 4], [6, 7, 8], [9, 9, 8]])
    out = _run_components(amd, faces, 11)
    assert out["vertex_label"].tolist() == [0, 1, 1, 1, 1, 5, 6, 6, 6, 6, 10]
    assert out["face_label"].tolist() == [6, 1, 1, 6, 6]
    assert out["table"][:, :5].tolist() == [[0, 1, 5, 6, 10], [0, 2, 0, 3, 0], [1, 4, 1, 4, 1]]
    _assert_components(out, M.components_reference(faces, 11))


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_components_of_one_chain(amd, order):
    """A triangle strip is one component whatever the numbering; under a permutation the parent chains are deep and cross wave and
    block boundaries.  Sizes around one wave (64), one block (256), and 391 blocks."""
    for n in (3, 63, 64, 65, 255, 256, 257, 100003):
        faces = _strip(_numbering(order, n))
        out = _run_components(amd, faces, n)
        assert out["C"] == 1 and out["table"][:, 0].tolist() == [0, n - 2, n], n
        assert bool((out["vertex_label"] == 0).all()) and bool((out["face_label"] == 0).all()), n


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_components_of_two_interleaved_chains(amd, order):
    for n in (3, 64, 257, 50001):
        ids = _numbering(order, n)
        faces = np.concatenate([_strip(2 * ids), _strip(2 * ids + 1)])
        faces = faces[np.random.default_rng(n).permutation(len(faces))]          # neighbouring threads work on both chains
        out = _run_components(amd, faces, 2 * n)
        assert out["C"] == 2 and out["table"][:, :2].tolist() == [[0, 1], [n - 2, n - 2], [n, n]], n
        assert np.array_equal(out["vertex_label"].cpu().numpy(), np.arange(2 * n) % 2), n
        assert np.array_equal(out["face_label"].cpu().numpy(), faces[:, 0] % 2), n


# ---- 3. the out-of-range guard ---------------------------------------------------------------------------------------------------------
def test_components_out_of_range_faces_join_nothing(amd):
    _, v, t = _case("two_spheres", (9, 12, 17))
    V = len(v)
    ref = _components("two_spheres", (9, 12, 17))
    a, b = int(np.flatnonzero(ref[0] == ref[2][0][0])[3]), int(np.flatnonzero(ref[0] == ref[2][0][1])[3])     # one vertex of each sphere
    bad = np.array([[a, b, V], [a, -1, b], [2 ** 31 - 1, a, b], [a, b, -2 ** 31]], dtype=np.int32)          # would join the spheres
    faces = np.concatenate([t[:100], bad[:2], t[100:], bad[2:]])
    out = _run_components(amd, faces, V)                                        # (checks the sentinels around labels and workspace)
    where = np.array([100, 101, len(faces) - 2, len(faces) - 1])
    got_fl = out["face_label"].cpu().numpy()
    assert (got_fl[where] == -1).all()
    assert np.array_equal(out["vertex_label"].cpu().numpy(), ref[0])
    assert np.array_equal(np.delete(got_fl, where), ref[1])
    for row, want in zip(out["table"], ref[2]):
        assert np.array_equal(row[:out["C"]].cpu().numpy(), want)
    assert np.array_equal(got_fl, M.components_reference(faces, V)[1])
    # the filter never keeps them
    vertices = torch.from_numpy(np.array(v)).cuda()
    v2, f2, idx = amd.filter_components(vertices, out["faces"], min_triangles=0)
    assert torch.equal(v2, vertices) and np.array_equal(f2.cpu().numpy(), t) and idx.tolist() == list(range(V))


# ---- 4. the filter against the restatement -------------------------------------------------------------------------------------------
def _run_filter(amd, comp, vertices, keep_labels):
    """nerf_mesh_filter_count / _emit through the C ABI on the labels of `comp`, keeping the components in keep_labels; outputs
    oversized and sentinel-filled -> (V', T', vertices buffer, faces buffer, vertex_index buffer)."""
    L = amd._lib
    V, T = comp["V"], comp["T"]
    keep = torch.zeros(V, dtype=torch.uint8, device="cuda")
    keep[torch.tensor(sorted(keep_labels), dtype=torch.int64, device="cuda")] = 1
    counts = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
    L.call("nerf_mesh_filter_count", comp["vertex_label"], comp["face_label"], keep, V, T, comp["workspace"], counts)
    n_v, n_t = counts.tolist()
    vbuf = torch.full((n_v + PAD, 3), 12345.0, device="cuda")
    fbuf = torch.full((n_t + PAD, 3), SENTINEL, dtype=torch.int32, device="cuda")
    ibuf = torch.full((n_v + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    L.call("nerf_mesh_filter_emit", vertices, comp["faces"], V, T, comp["workspace"], vbuf, fbuf, ibuf)
    torch.cuda.synchronize()
    assert bool((vbuf[n_v:] == 12345.0).all() and (fbuf[n_t:] == SENTINEL).all() and (ibuf[n_v:] == SENTINEL).all())
    return n_v, n_t, vbuf, fbuf, ibuf


def _assert_filter(amd, comp, v, t, ref, **criteria):
    table = ref[2]
    ref_v, ref_f, ref_i = M.filter_reference(v, t, components=ref, **criteria)
    vertices = torch.from_numpy(np.array(v)).cuda()
    n_v, n_t, vbuf, fbuf, ibuf = _run_filter(amd, comp, vertices, M.select_reference(table, **criteria))
    assert (n_v, n_t) == (len(ref_v), len(ref_f))
    assert np.array_equal(fbuf[:n_t].cpu().numpy(), ref_f) and np.array_equal(ibuf[:n_v].cpu().numpy(), ref_i)
    assert np.array_equal(_bits(vbuf[:n_v].cpu().numpy()), _bits(ref_v))
    v2, f2, idx = amd.filter_components(vertices, comp["faces"], **criteria)     # the Python interface: its own choice of rows
    assert v2.dtype == torch.float32 and f2.dtype == idx.dtype == torch.int32
    assert v2.shape == (n_v, 3) and f2.shape == (n_t, 3) and idx.shape == (n_v,)
    assert torch.equal(f2, fbuf[:n_t]) and torch.equal(idx, ibuf[:n_v]) and torch.equal(v2.view(torch.int32), vbuf[:n_v].view(torch.int32))
    assert torch.equal(v2.view(torch.int32), vertices[idx.long()].view(torch.int32))
    return v2, f2, idx


def test_filter_ties_on_the_random_field(amd):
    name, shape = "random", (33, 33, 33)
    _, v, t = _case(name, shape)
    ref = _components(name, shape)
    table = ref[2]
    sizes = sorted(table[1].tolist(), reverse=True)
    tied = table[0][table[1] == 24]                                             # ascending labels
    assert sizes[:4] == [245752, 24, 24, 24] and len(sizes) == 17 and 3 <= len(tied) < 16 and sizes[1 + len(tied)] < 24
    comp = _run_components(amd, t, len(v))
    giant = int(table[0][np.argmax(table[1])])
    for k in (1, 2, 3, 4, len(tied) + 1, len(tied) + 2):                        # through the ties, and one past them
        assert M.select_reference(table, keep_largest=k) >= {giant} | set(tied[:k - 1].tolist())
        assert len(M.select_reference(table, keep_largest=k)) == k and (k > len(tied) or not set(tied[k - 1:].tolist()) & M.select_reference(table, keep_largest=k))
        _assert_filter(amd, comp, v, t, ref, keep_largest=k)
    for k in (17, 18, 10 ** 6):                                                 # keep_largest >= C: the identity
        v2, f2, idx = _assert_filter(amd, comp, v, t, ref, keep_largest=k)
        assert np.array_equal(f2.cpu().numpy(), t) and idx.tolist() == list(range(len(v)))
    _assert_filter(amd, comp, v, t, ref, min_triangles=24)                    # the giant and the 24s
    _assert_filter(amd, comp, v, t, ref, min_triangles=25)
    _assert_filter(amd, comp, v, t, ref, min_triangles=24, keep_largest=3)    # both must hold
    _assert_filter(amd, comp, v, t, ref, min_triangles=2, keep_largest=16)
    for nothing in ({"min_triangles": 245753}, {"keep_largest": 0}):
        v2, f2, idx = _assert_filter(amd, comp, v, t, ref, **nothing)
        assert v2.shape == (0, 3) and f2.shape == (0, 3) and idx.shape == (0,)


@pytest.mark.parametrize("name,shape", [("two_spheres", (9, 12, 17)), ("sinusoids", (33, 33, 33)), ("random", (67, 63, 66))])
def test_filter_at_a_components_size(amd, name, shape):
    """min_triangles at exactly a component's size keeps it, one more drops it."""
    _, v, t = _case(name, shape)
    ref = _components(name, shape)
    table = ref[2]
    comp = _run_components(amd, t, len(v))
    sizes = sorted(set(table[1].tolist()))
    for m in (sizes[-1], sizes[-1] + 1, sizes[-2], sizes[-2] + 1):
        kept = M.select_reference(table, min_triangles=m)
        assert len(kept) == int((table[1] >= m).sum())
        _assert_filter(amd, comp, v, t, ref, min_triangles=m)
    _assert_filter(amd, comp, v, t, ref, keep_largest=2)


# ---- 5. filtered topology ------------------------------------------------------------------------------------------------------------
def test_filtered_sphere_is_a_closed_surface(amd):
    _, v, t = _case("two_spheres", (33, 33, 33))
    whole = R.mesh_stats(v, t)
    assert whole["closed"] and whole["euler"] == 4
    v2, f2, _ = amd.filter_components(torch.from_numpy(np.array(v)).cuda(), torch.from_numpy(np.array(t)).cuda(), keep_largest=1)
    st = R.mesh_stats(v2.cpu().numpy(), f2.cpu().numpy())
    assert st["T"] == 2584 and st["closed"] and st["oriented"] and st["euler"] == 2 and st["used_all_vertices"] and st["volume"] > 0


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_components_refuse_more_than_int32_elements(amd):
    """Through the size checks alone: nothing is allocated, no pointer is read, nothing is launched."""
    lib = amd._lib.load()
    big = 2 ** 31
    for v, t in ((big, 1), (1, big)):
        assert lib.nerf_mesh_components_workspace_bytes(v, t) == -1
        assert lib.nerf_mesh_components(None, t, v, None, None, None, None, None, None, None, None) == -1
        assert b"2^31" in lib.nerf_last_error()
        assert lib.nerf_mesh_filter_count(None, None, None, v, t, None, None, None) == -1
        assert b"2^31" in lib.nerf_last_error()
        assert lib.nerf_mesh_filter_emit(None, None, v, t, None, None, None, None, None) == -1
    assert lib.nerf_mesh_components_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) > 0
    torch.cuda.synchronize()


# ---- 7. vertex_colors ----------------------------------------------------------------------------------------------------------------
def _points_and_dirs(n=200, seed=7):
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=gen) * 2.4 - 1.2).contiguous()
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return pts, (d / d.norm(dim=-1, keepdim=True)).to(torch.float32).contiguous()


def test_vertex_colors_f32_against_the_oracle(amd, oracle, synthetic_sd):
    """bound: max|d c| <= 1/4 * 2e-5 * max|raw_ref| over the colour channels -- DESIGN 3.1's fp32 raw tolerance times the sigmoid's
    largest slope."""
    net = network(amd, synthetic_sd, "f32", train=False)
    pts, dirs = _points_and_dirs()
    col = amd.vertex_colors(net, pts.cuda(), dirs.cuda())
    assert col.shape == (200, 3) and col.dtype == torch.float32 and col.is_cuda
    assert bool((col >= 0).all() and (col <= 1).all())
    raw_ref = oracle.network_forward(synthetic_sd, pts[:, None, :], dirs, model="fine")[:, 0, :3].double()
    err = (col.cpu().double() - torch.sigmoid(raw_ref)).abs().max().item()
    bound = 0.25 * 2e-5 * raw_ref.abs().max().item()
    print(f"vertex_colors f32 vs oracle: max|d c| = {err:.3e}, bound = {bound:.3e}, max|raw_ref rgb| = {raw_ref.abs().max().item():.3e}")
    assert err <= bound
    coarse = amd.vertex_colors(net, pts.cuda(), dirs.cuda(), model="")
    assert torch.equal(coarse, torch.sigmoid(net.forward(pts.cuda()[:, None, :], dirs.cuda(), None, model="")[:, 0, :3]))
    assert amd.vertex_colors(net, torch.zeros((0, 3), device="cuda")).shape == (0, 3)


def test_vertex_colors_default_direction_is_against_the_normal(amd, synthetic_sd):
    net = network(amd, synthetic_sd, "f32", train=False)
    pts, _ = _points_and_dirs(96, seed=8)
    pts = pts.cuda()
    n = amd.vertex_normals(net, pts)
    assert bool((n.norm(dim=-1) > 0.5).all())
    assert torch.equal(amd.vertex_colors(net, pts), amd.vertex_colors(net, pts, -n))
    assert torch.equal(amd.vertex_colors(net, pts, model=""), amd.vertex_colors(net, pts, -amd.vertex_normals(net, pts, model=""), model=""))


@pytest.mark.parametrize("precision", ["f16", "f32x"])
def test_vertex_colors_other_precisions_are_the_mlp_forward(amd, synthetic_sd, precision):
    L = amd._lib
    net = network(amd, synthetic_sd, precision, train=False)
    pts, dirs = _points_and_dirs()
    pts, dirs = pts.cuda(), dirs.cuda()
    raw = torch.empty(200, 1, 4, device="cuda")
    L.call("nerf_mlp_forward", pts, dirs, 200, 1, net.packed("fine"), raw, L.PRECISIONS[precision])
    assert torch.equal(amd.vertex_colors(net, pts, dirs), torch.sigmoid(raw[:, 0, :3]))


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    """-> x y z [V,3], nx ny nz [V,3], red green blue [V,3] uint8, faces [T,3] of a PLY with exactly those properties."""
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    n_v, n_f = int(lines[2].split()[-1]), int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2] == f"element vertex {n_v}"
    assert lines[3:12] == [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {p}" for p in ("red", "green", "blue")]
    assert lines[12:] == [f"element face {n_f}", "property list uchar int vertex_indices", ""]
    assert len(body) == 27 * n_v + 13 * n_f
    rows = [struct.unpack_from("<6f3B", body, 27 * k) for k in range(n_v)]
    rows = np.array(rows, dtype=np.float64).reshape(n_v, 9)
    faces = np.array([struct.unpack_from("<Biii", body, 27 * n_v + 13 * k) for k in range(n_f)], dtype=np.int64).reshape(n_f, 4)
    assert (faces[:, 0] == 3).all()
    return rows[:, :3].astype(np.float32), rows[:, 3:6].astype(np.float32), rows[:, 6:].astype(np.uint8), faces[:, 1:].astype(np.int32)


def test_extract_mesh_filtered_with_normals_and_colours(amd, family_sd, tmp_path):
    from nerf_replication_amd.mesh import grid_axes
    net = network(amd, family_sd("trained"), "f32", train=False)
    box, n = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], 48
    grid = amd.density_grid(net, box, n)
    level = 0.5 * (grid.median().item() + grid.max().item())            # the level rule of test_extract_mesh_end_to_end
    _, origin, step = grid_axes(box, n)
    # the reference comes from the GPU's own grid, through the two restatements
    ref_v, ref_t, _ = R.isosurface_reference(grid.cpu().numpy(), level, origin, step)
    table = M.components_reference(ref_t, len(ref_v))[2]
    print(f"trained 48^3: {len(ref_v)} vertices, {len(ref_t)} triangles, {len(table[0])} components, largest {sorted(table[1].tolist())[-6:]}")
    assert len(table[0]) > 1
    want_v, want_f, want_i = M.filter_reference(ref_v, ref_t, keep_largest=1)
    assert len(want_f) == table[1].max()

    path = str(tmp_path / "clean.ply")
    v1, f1 = amd.extract_mesh(net, level, box, path, n, normals=True, keep_largest=1, colors=True)
    assert np.array_equal(f1.cpu().numpy(), want_f) and np.array_equal(_bits(v1.cpu().numpy()), _bits(want_v))
    normals = amd.vertex_normals(net, v1)
    colors = amd.vertex_colors(net, v1)
    assert torch.equal(colors, amd.vertex_colors(net, v1, -normals))
    pv, pn, pc, pf = _read_ply(path)
    assert np.array_equal(_bits(pv), _bits(v1.cpu().numpy())) and np.array_equal(pf, want_f)
    assert np.array_equal(_bits(pn), _bits(normals.cpu().numpy()))
    assert np.array_equal(pc, np.floor(np.clip(colors.cpu().numpy().astype(np.float64), 0, 1) * 255 + 0.5).astype(np.uint8))
    assert pc.std() > 0                                                  # (not one constant colour)

    # with the new arguments at their defaults the file is what isosurface + write_ply give
    plain, direct = str(tmp_path / "plain.ply"), str(tmp_path / "direct.ply")
    v0, f0 = amd.extract_mesh(net, level, box, plain, n)
    assert np.array_equal(f0.cpu().numpy(), ref_t) and np.array_equal(_bits(v0.cpu().numpy()), _bits(ref_v))
    amd.write_ply(direct, *amd.isosurface(grid, level, origin, step))
    assert open(plain, "rb").read() == open(direct, "rb").read()
    # min_triangles alone, and an array of colours passed through
    size = int(np.sort(table[1])[-2])
    v3, f3 = amd.extract_mesh(net, level, box, path, n, min_triangles=size, colors=None)
    want3 = M.filter_reference(ref_v, ref_t, min_triangles=size)
    assert np.array_equal(f3.cpu().numpy(), want3[1]) and np.array_equal(_bits(v3.cpu().numpy()), _bits(want3[0]))
