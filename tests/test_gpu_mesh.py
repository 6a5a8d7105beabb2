"""GPU tests of the mesh feature (nerf_replication_amd/mesh.py): the nerf_isosurface_* kernels against the NumPy restatement
tests/isosurface_reference.py (faces exactly, vertices bit for bit), density_grid against the point-mode / ray-mode MLP entries
and the CPU oracle, and extract_mesh end to end on the trained checkpoint."""
import functools
import os

import numpy as np
import pytest
import torch

import isosurface_reference as R
from gpu_common import amd, network  # noqa: F401

pytestmark = pytest.mark.gpu

# The scan has two levels: 256 points per block (nerf_isosurface_count_kernel), then one workgroup of 1024 threads over the
# block totals, each thread taking ceil(n_blocks / 1024) consecutive blocks (nerf_isosurface_scan_kernel).  One pass of both
# levels covers 1024 * 256 = 262 144 points; 67 x 63 x 66 = 278 586 points are 1089 blocks, two per scan thread, ragged at
# the end of both levels.
BIG = (67, 63, 66)
SHAPES = [(2, 2, 2), (9, 12, 17), (33, 33, 33), BIG]
FIELDS = ["sphere", "two_spheres", "torus", "sinusoids", "random"]
V_SENTINEL, T_SENTINEL, PAD = 12345.0, -7, 5


@functools.lru_cache(maxsize=None)
def _case(name, shape):
    f = R.analytic_field(name, shape)
    f.setflags(write=False)
    v, t, _ = R.isosurface_reference(f, R.LEVELS[name], R.BOX_ORIGIN, R.box_step(shape))
    return f, v, t


def _device_field(f, stride):
    """The grid on the device: dense, or as the sigma column of a NaN-filled [nx,ny,nz,4] raw buffer."""
    if stride == 1:
        return torch.from_numpy(np.array(f)).cuda()
    raw = torch.full(f.shape + (4,), float("nan"), device="cuda")
    raw[..., 3] = torch.from_numpy(np.array(f)).cuda()
    return raw[..., 3]


def _run_abi(amd, field, level, origin, step):
    """count + emit through the C ABI into oversized, sentinel-filled buffers -> (V, T, vertices buffer, triangles buffer)."""
    L = amd._lib
    nx, ny, nz = field.shape
    stride = field.stride(2)
    ws = torch.empty(int(L.call("nerf_isosurface_workspace_bytes", nx, ny, nz)), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -99, dtype=torch.int32, device="cuda")
    L.call("nerf_isosurface_count", L.strided(field), stride, nx, ny, nz, level, ws, counts)
    n_v, n_t = counts.tolist()
    vbuf = torch.full((n_v + PAD, 3), V_SENTINEL, device="cuda")
    tbuf = torch.full((n_t + PAD, 3), T_SENTINEL, dtype=torch.int32, device="cuda")
    L.call("nerf_isosurface_emit", L.strided(field), stride, nx, ny, nz, level, origin, step, ws, vbuf, tbuf)
    torch.cuda.synchronize()
    return n_v, n_t, vbuf, tbuf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", FIELDS)
def test_isosurface_equals_the_restatement(amd, name, shape):
    f, ref_v, ref_t = _case(name, shape)
    level, origin, step = R.LEVELS[name], R.BOX_ORIGIN, R.box_step(shape)
    for stride in (1, 4):
        field = _device_field(f, stride)
        assert field.stride(2) == stride
        n_v, n_t, vbuf, tbuf = _run_abi(amd, field, level, origin, step)
        assert (n_v, n_t) == (len(ref_v), len(ref_t))                       # what count announced is what emit wrote
        assert (vbuf[n_v:] == V_SENTINEL).all() and (tbuf[n_t:] == T_SENTINEL).all()
        assert np.array_equal(tbuf[:n_t].cpu().numpy(), ref_t)
        assert np.array_equal(_bits(vbuf[:n_v].cpu().numpy()), _bits(ref_v))
        again = _run_abi(amd, field, level, origin, step)                   # no atomics: the same bytes
        assert torch.equal(again[2], vbuf) and torch.equal(again[3], tbuf)
        v, t = amd.isosurface(field, level, origin, step)                   # the Python interface
        assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape == (n_v, 3) and t.shape == (n_t, 3)
        assert torch.equal(t, tbuf[:n_t]) and torch.equal(v.view(torch.int32), vbuf[:n_v].view(torch.int32))
    if name == "sphere" and shape == (33, 33, 33):
        st = R.mesh_stats(v.cpu().numpy(), t.cpu().numpy())
        assert st["closed"] and st["oriented"] and st["euler"] == 2 and st["volume"] > 0


def test_isosurface_raw_buffer_argument(amd):
    """A 4-D [nx,ny,nz,4] raw buffer is read in place: sigma is channel 3."""
    f, ref_v, ref_t = _case("torus", (9, 12, 17))
    raw = torch.zeros(f.shape + (4,), device="cuda")
    raw[..., 3] = torch.from_numpy(np.array(f)).cuda()
    v, t = amd.isosurface(raw, 0.0, R.BOX_ORIGIN, R.box_step(f.shape))
    assert np.array_equal(t.cpu().numpy(), ref_t) and np.array_equal(_bits(v.cpu().numpy()), _bits(ref_v))
    with pytest.raises(ValueError):
        amd.isosurface(raw[..., 3].permute(2, 1, 0), 0.0, R.BOX_ORIGIN, R.box_step(f.shape))
    with pytest.raises(amd._lib.NerfLibraryError):
        amd.isosurface(torch.zeros(3, 3, 3), 0.0, R.BOX_ORIGIN, (1, 1, 1))


def test_isosurface_empty_results(amd):
    L = amd._lib
    f = torch.from_numpy(np.array(_case("sphere", (9, 12, 17))[0])).cuda()
    for field, level in ((f, 10.0), (f, -10.0), (f[:1].contiguous(), 0.0), (f[:, :1].contiguous(), 0.0), (f[:, :, :1].contiguous(), 0.0)):
        v, t = amd.isosurface(field, level, R.BOX_ORIGIN, (0.1, 0.1, 0.1))
        assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32
        nx, ny, nz = field.shape
        counts = torch.full((2,), -99, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(1, int(L.call("nerf_isosurface_workspace_bytes", nx, ny, nz))), dtype=torch.uint8, device="cuda")
        L.call("nerf_isosurface_count", field, 1, nx, ny, nz, level, ws, counts)
        assert counts.tolist() == [0, 0]


def test_isosurface_level_ties_and_nans(amd):
    """Inside iff f > level: a value equal to the level is outside (tau is then exactly 0 or 1), NaN is outside (its vertices are
    NaN).  Faces exactly; vertices bit for bit where finite, NaN where the restatement has NaN (payloads are not compared)."""
    rng = np.random.default_rng(5)
    f = np.array(_case("random", (9, 12, 17))[0])
    pick = rng.random(f.shape)
    f[pick < 0.10] = 0.5
    f[pick > 0.95] = np.nan
    ref_v, ref_t, _ = R.isosurface_reference(f, 0.5, R.BOX_ORIGIN, R.box_step(f.shape))
    assert np.isnan(ref_v).any() and len(ref_t) > 0
    for stride in (1, 4):
        n_v, n_t, vbuf, tbuf = _run_abi(amd, _device_field(f, stride), 0.5, R.BOX_ORIGIN, R.box_step(f.shape))
        assert (n_v, n_t) == (len(ref_v), len(ref_t))
        assert np.array_equal(tbuf[:n_t].cpu().numpy(), ref_t)
        got = vbuf[:n_v].cpu().numpy()
        nan = np.isnan(ref_v)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(ref_v)[~nan])
        assert (vbuf[n_v:] == V_SENTINEL).all() and (tbuf[n_t:] == T_SENTINEL).all()


def test_isosurface_refuses_more_than_int32_points(amd):
    """Through the size checks alone: nothing is allocated and no pointer is read."""
    lib, L = amd._lib.load(), amd._lib
    assert lib.nerf_isosurface_workspace_bytes(2048, 2048, 512) == -1                  # 2^31 points
    assert lib.nerf_isosurface_workspace_bytes(-1, 4, 4) == -1
    n = 1290 ** 3                                                                       # 2 146 689 000 < 2^31 - 1
    blocks = (n + 255) // 256
    assert lib.nerf_isosurface_workspace_bytes(1290, 1290, 1290) == (4 * n + 255) // 256 * 256 + 2 * ((4 * blocks + 255) // 256 * 256)
    assert lib.nerf_isosurface_count(None, 1, 2048, 2048, 512, 0.0, None, None, None) == -1
    assert b"2^31" in lib.nerf_last_error()
    assert lib.nerf_isosurface_emit(None, 1, 2048, 2048, 512, 0.0, None, None, None, None, None, None) == -1
    assert lib.nerf_isosurface_count(None, 0, 4, 4, 4, 0.0, None, None, None) == -1    # stride < 1


# ---- density_grid ---------------------------------------------------------------------------------------------------------------
BOX = [-1.2, -0.8, -1.5, 1.1, 0.9, 1.4]
DIMS = (8, 6, 10)


def _grid_points():
    from nerf_replication_amd.mesh import grid_axes
    axes, _, _ = grid_axes(BOX, DIMS)
    x, y, z = (torch.from_numpy(a.astype(np.float32)) for a in axes)
    pts = torch.stack(torch.meshgrid(x, y, z, indexing="ij"), dim=-1).reshape(DIMS[0] * DIMS[1], DIMS[2], 3)
    vd = torch.tensor([[0.0, 0.0, 1.0]]).expand(pts.shape[0], 3).contiguous()
    return pts, vd, z


def test_density_grid_f32_is_the_point_mode_sigma(amd, oracle, synthetic_sd):
    net = network(amd, synthetic_sd, "f32", train=False)
    pts, vd, _ = _grid_points()
    grid = amd.density_grid(net, BOX, DIMS)
    assert grid.shape == DIMS and grid.dtype == torch.float32 and grid.is_cuda and grid.is_contiguous()
    raw = net.forward(pts.cuda(), vd.cuda(), None, model="fine")
    assert torch.equal(grid.reshape(-1, DIMS[2]), raw[..., 3])                     # the ray / point identity
    ref = oracle.network_forward(synthetic_sd, pts, vd, model="fine")[..., 3]
    err = (grid.cpu().reshape(-1, DIMS[2]).double() - ref.double()).abs().max().item()
    print(f"density_grid f32 vs oracle: max|d sigma| = {err:.3e}, max|ref| = {ref.abs().max().item():.3e}")
    assert err <= 2e-5 * ref.abs().max().item()                                     # DESIGN 3.1's fp32 raw tolerance
    assert torch.equal(amd.density_grid(net, BOX, DIMS, chunk_lines=7), grid)       # 48 lines: six chunks of 7 and one of 6
    coarse = amd.density_grid(net, BOX, DIMS, model="")
    assert torch.equal(coarse.reshape(-1, DIMS[2]), net.forward(pts.cuda(), vd.cuda(), None, model="")[..., 3])


@pytest.mark.parametrize("precision", ["f16", "f32x", "f16m32"])
def test_density_grid_other_precisions_are_the_ray_mode_sigma(amd, synthetic_sd, precision):
    L = amd._lib
    net = network(amd, synthetic_sd, precision, train=False)
    pts, vd, z = _grid_points()
    o = pts[:, 0, :].clone()
    o[:, 2] = 0.0
    o, d, t = o.cuda(), vd.cuda(), z.cuda()
    full = torch.empty(pts.shape[0], DIMS[2], 4, device="cuda")
    L.call("nerf_mlp_forward_rays", o, d, t, 0, pts.shape[0], DIMS[2], net.packed("fine"), full, L.PRECISIONS[precision])
    grid = amd.density_grid(net, BOX, DIMS)
    assert torch.equal(grid.reshape(-1, DIMS[2]), full[..., 3])
    assert torch.equal(amd.density_grid(net, BOX, DIMS, chunk_lines=7), grid)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    n_v = int(lines[2].split()[-1])
    n_f = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert len(body) == 12 * n_v + 13 * n_f
    v = np.frombuffer(body[:12 * n_v], dtype="<f4").reshape(n_v, 3)
    f = np.frombuffer(body[12 * n_v:], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert (f["n"] == 3).all()
    return v, f["i"]


def test_extract_mesh_end_to_end(amd, family_sd, tmp_path):
    net = network(amd, family_sd("trained"), "f32", train=False)
    box, n = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], 48
    grid = amd.density_grid(net, box, n)
    level = 0.5 * (grid.median().item() + grid.max().item())            # from the grid itself: the surface is not empty
    from nerf_replication_amd.mesh import grid_axes
    _, origin, step = grid_axes(box, n)
    v0, t0 = amd.isosurface(grid, level, origin, step)
    assert len(t0) > 0 and int(t0.max()) < len(v0) and int(t0.min()) >= 0
    path = str(tmp_path / "net.ply")
    v1, t1 = amd.extract_mesh(net, level, box, path, n)
    assert torch.equal(t1, t0) and torch.equal(v1.view(torch.int32), v0.view(torch.int32))
    pv, pf = _read_ply(path)
    assert np.array_equal(_bits(pv), _bits(v1.cpu().numpy())) and np.array_equal(pf, t1.cpu().numpy())

    # the reference's protocol: a callable on explicit points.  In f32 point mode and ray mode give bit-equal sigma on bit-equal
    # points (test_density_grid_f32_is_the_point_mode_sigma), so the bound on the vertex difference is zero.
    calls = []

    def queryfn(xyz):
        calls.append(xyz.shape[0])
        assert xyz.is_cuda and xyz.dim() == 2 and xyz.shape[1] == 3
        vd = torch.tensor([[0.0, 0.0, 1.0]], device=xyz.device).expand(xyz.shape[0], 3).contiguous()
        return net(xyz[:, None, :], vd, None, "fine")[:, 0, 3:4]
    path2 = str(tmp_path / "fn.ply")
    v2, t2 = amd.extract_mesh(queryfn, level, box, path2, n)
    assert sum(calls) == n ** 3
    assert torch.equal(t2, t0)
    print("callable protocol: max|d vertex| =", (v2 - v0).abs().max().item())
    assert torch.equal(v2.view(torch.int32), v0.view(torch.int32))
    assert open(path2, "rb").read() == open(path, "rb").read()
