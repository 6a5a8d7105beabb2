"""GPU tests of the occupancy grid (nerf_replication_amd/occupancy.py): the nerf_occupancy_* kernels against
the NumPy restatement tests/occupancy_reference.py (byte for byte), and the culled render against the plain render: bit-equal on
every ray none of whose culled samples has a positive density, which the staged entries decide."""
import functools

import numpy as np
import pytest
import torch

import isosurface_reference as R
import occupancy_reference as O
from conftest import parity_record
from gpu_common import amd, network  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -1412567297, 6            # 0xABCDEEFF as int32
BOX = [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0]
BIG_BOX = [-8.0, -8.0, -8.0, 8.0, 8.0, 8.0]          # contains every sample: |o| = 4.03, t <= 6 (t_sorted <= 6 too)
N_PROBE = 512


# ---- 1. build ---------------------------------------------------------------------------------------------------------------------
def _device_field(f, stride):
    if stride == 1:
        return torch.from_numpy(np.array(f)).cuda()
    raw = torch.full(f.shape + (4,), float("nan"), device="cuda")            # NaN in the channels that must not be read
    raw[..., 3] = torch.from_numpy(np.array(f)).cuda()
    return raw[..., 3]


def _build_abi(amd, field, level, dilate):
    L = amd._lib
    nx, ny, nz = field.shape
    n_words = int(L.call("nerf_occupancy_words", nx, ny, nz))
    buf = torch.full((n_words + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    L.call("nerf_occupancy_build", L.strided(field), field.stride(2), nx, ny, nz, level, dilate, buf)
    torch.cuda.synchronize()
    assert (buf[n_words:] == SENTINEL).all()
    return buf[:n_words].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", [(9, 12, 17), (33, 33, 33)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,level", [("torus", 0.0), ("sphere", 0.0), ("sphere", 0.125), ("torus", -0.25)])
def test_build_equals_the_restatement(amd, name, level, shape):
    """(9,12,17): 1408 cells, a ragged last word; (33,33,33): 32 768 cells, a multiple of 64.  dilate 0, 1, 2; dense and as the
    sigma column of a raw buffer; one NaN point."""
    f = R.analytic_field(name, shape)
    f_nan = np.array(f)
    f_nan[tuple(n // 3 for n in shape)] = np.nan
    for field_np, dilates in ((f, (0, 1, 2)), (f_nan, (1,))):
        for dilate in dilates:
            ref = O.build(field_np, level, dilate)
            n_cells = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
            assert 0 < np.unpackbits(ref.view(np.uint8)).sum() < n_cells           # neither empty nor full: the case says something
            for stride in (1, 4):
                field = _device_field(field_np, stride)
                assert field.stride(2) == stride
                got = _build_abi(amd, field, level, dilate)
                assert got.shape == ref.shape and np.array_equal(got, ref), (name, level, shape, dilate, stride)
                assert np.array_equal(_build_abi(amd, field, level, dilate), got)       # no atomics: the same bytes
            grid = amd.OccupancyGrid.from_fields([-1, -1, -1, 1, 1, 1], fine=_device_field(field_np, 4), level=level, dilate=dilate)
            cells = O.cells(field_np, level, dilate)
            assert grid.bits[""] is None and np.array_equal(grid.bits["fine"].cpu().numpy().view(np.uint32), ref)
            got_cells = grid.cells("fine")
            assert got_cells.dtype == torch.bool and got_cells.shape == cells.shape and np.array_equal(got_cells.cpu().numpy(), cells)
            assert grid.occupied_fraction("fine") == pytest.approx(cells.mean(), abs=1e-6)
            with pytest.raises(ValueError):
                grid.cells("")
    assert (amd.OccupancyGrid.from_fields([-1, -1, -1, 1, 1, 1], coarse=torch.from_numpy(f).cuda(), dilate=10 ** 6).cells("")).all()


# ---- 2. mark ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probe_rays():
    import nerf_oracle
    ids = torch.from_numpy(np.random.default_rng(5).choice(800 * 800, N_PROBE, replace=False))
    o, d = nerf_oracle.pinhole_rays(800, 800, nerf_oracle.camera_pose(40.0), pixel_ids=ids)
    return o.cuda(), d.cuda()


def _mark_abi(amd, o, d, t, stride, S, bits, dims, lo, inv, and_with_existing, valid):
    amd._lib.call("nerf_occupancy_mark", o, d, t, stride, o.shape[0], S, bits, dims, lo.tolist(), inv.tolist(), and_with_existing, valid)
    torch.cuda.synchronize()
    return valid


@pytest.mark.parametrize("S", [64, 192])
def test_mark_equals_the_restatement(amd, S):
    """200 rays (neither a multiple of 64 nor of 256) from the probe camera through a torus grid on [-1.5, 1.5]^3: at least
    half of the rays enter and leave the box.  S = 64 reads the shared table (stride 0), S = 192 one row per ray; one ray is NaN."""
    n, dims, bbox = 200, (9, 12, 17), [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    o, d = (x[:n].clone() for x in _probe_rays())
    o[17, 1] = float("nan")
    words = O.build(R.analytic_field("torus", dims), 0.0, 1)
    lo, inv = O.lookup_frame(bbox, dims)
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    if S == 64:
        t, stride = torch.linspace(2.0, 6.0, 64).cuda(), 0
    else:
        g = torch.Generator().manual_seed(3)
        t, stride = (2.0 + 4.0 * torch.rand(n, S, generator=g)).sort(dim=1).values.cuda().contiguous(), S
    ref = O.keep(o.cpu().numpy(), d.cpu().numpy(), t.cpu().numpy(), words, dims, lo, inv)
    assert ref.shape == (n, S) and ref[17].all()
    x = o.cpu().numpy()[:, None, :] + d.cpu().numpy()[:, None, :] * np.broadcast_to(t.cpu().numpy(), (n, S))[:, :, None]
    outside = (np.abs(x) > 1.5).any(-1)
    assert (outside.any(axis=1) & (~outside).any(axis=1)).sum() >= n // 2              # rays that enter and leave the box
    assert (~ref).any() and (ref & ~outside).any()                                     # culled samples, and kept ones inside the box
    buf = torch.full((n * S + PAD,), 77, dtype=torch.uint8, device="cuda")
    got = _mark_abi(amd, o, d, t, stride, S, bits, dims, lo, inv, 0, buf)
    assert (got[n * S:] == 77).all()
    assert np.array_equal(got[:n * S].cpu().numpy().reshape(n, S), ref.astype(np.uint8))
    existing = torch.randint(0, 3, (n, S), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)      # 0, 1, 2: non-zero is valid
    got = _mark_abi(amd, o, d, t, stride, S, bits, dims, lo, inv, 1, existing.cuda().contiguous())
    assert np.array_equal(got.cpu().numpy(), ((existing.numpy() != 0) & ref).astype(np.uint8))


# ---- 3. render exactness ------------------------------------------------------------------------------------------------------------
def _render(amd, net, o, d, grid=None, n_importance=128, fast=False, threshold=0.25):
    """-> rgb, depth, evaluated (a list of two ints, None without a grid)"""
    r = amd.Renderer(net)
    r.N_importance, r.fast_sampling, r.weights_threshold = n_importance, fast, threshold
    r.occupancy = grid
    if grid is not None:
        r.occupancy_stats = []
    with torch.no_grad():
        rgb, dep = r.render({"rays_o": o[None], "rays_d": d[None]})
    if grid is None:
        assert r.occupancy_stats is None
        return rgb, dep, None
    (evaluated, total), = r.occupancy_stats
    assert evaluated.dtype == torch.int64 and evaluated.is_cuda and total == (64 * o.shape[0], 192 * o.shape[0])
    return rgb, dep, evaluated.tolist()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_SCENES = {}


@pytest.fixture
def scene(amd, family_sd):
    """(family, precision) -> the network, its grid (N = 64, dilate 1, on [-2,2]^3), the plain and the culled render of the 512 probe
    rays, and which rays are excluded: computed once, shared by the tests below, left unchanged."""
    def get(family, precision):
        key = (family, precision)
        if key not in _SCENES:
            L = amd._lib
            net = network(amd, family_sd(family), precision, train=False)
            o, d = _probe_rays()
            n, prec = o.shape[0], L.PRECISIONS[precision]
            grid = amd.OccupancyGrid.from_network(net, BOX, 64, dilate=1)
            assert grid.dims == (64, 64, 64) and grid.bits[""] is not None and grid.bits["fine"] is not None
            # the plain stages, one by one
            t_c, u = torch.linspace(2.0, 6.0, 64).cuda(), torch.linspace(0.0, 1.0, 128).cuda()
            raw_c = torch.empty(n, 64, 4, device="cuda")
            L.call("nerf_mlp_forward_rays_density", o, d, t_c, 0, n, 64, net.packed(""), raw_c, prec)
            t_sorted = torch.empty(n, 192, device="cuda")
            L.call("nerf_sample_fine", raw_c, t_c, u, n, t_sorted, None, None, 0.0, 0.0)
            raw_f = torch.empty(n, 192, 4, device="cuda")
            L.call("nerf_mlp_forward_rays", o, d, t_sorted, 192, n, 192, net.packed("fine"), raw_f, prec)
            # the two marks
            lo, inv = O.lookup_frame(BOX, grid.dims)
            assert np.array_equal(lo, grid.box_min) and np.array_equal(inv, grid.inv_step)
            keep_c = _mark_abi(amd, o, d, t_c, 0, 64, grid.bits[""], grid.dims, lo, inv, 0, torch.empty(n, 64, dtype=torch.uint8, device="cuda")).bool()
            keep_f = _mark_abi(amd, o, d, t_sorted, 192, 192, grid.bits["fine"], grid.dims, lo, inv, 0,
                               torch.empty(n, 192, dtype=torch.uint8, device="cuda")).bool()
            # excluded: a culled sample with sigma > 0 (coarse: it moves the fine samples; fine: it carries weight)
            excluded = (~keep_c & (raw_c[..., 3] > 0)).any(1) | (~keep_f & (raw_f[..., 3] > 0)).any(1)
            plain = _render(amd, net, o, d)
            culled = _render(amd, net, o, d, grid)
            _SCENES[key] = dict(net=net, grid=grid, o=o, d=d, keep_c=keep_c, keep_f=keep_f, excluded=excluded, plain=plain, culled=culled,
                                culled_coarse_positive=int((~keep_c & (raw_c[..., 3] > 0)).sum()),
                                culled_fine_positive=int((~keep_f & (raw_f[..., 3] > 0)).sum()))
        return _SCENES[key]
    return get


@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("family", ["trained", "sharp"])
def test_culled_render_is_bit_equal_where_no_positive_density_was_culled(scene, family, precision):
    """Bound on the excluded rays: 2 % of the 512 (the CPU probe with the oracle's grid: 3 / 512 on trained, 0 / 512 on sharp; the
    margin is for last-bit differences between the GPU grid and the oracle's).  The cull is not vacuous: at most half of the fine
    points are evaluated on both scenes (probe: 0.21 and 0.335), at most half of the coarse points on sharp (probe: 0.195)."""
    s = scene(family, precision)
    n = N_PROBE
    (rgb0, dep0, _), (rgb1, dep1, evaluated) = s["plain"], s["culled"]
    ex = s["excluded"]
    n_ex = int(ex.sum())
    d_rgb = (rgb1 - rgb0).abs().max(dim=1).values
    stats = dict(excluded_rays=n_ex, n_rays=n, culled_coarse_positive=s["culled_coarse_positive"], culled_fine_positive=s["culled_fine_positive"],
                 evaluated_coarse=evaluated[0] / (64 * n), evaluated_fine=evaluated[1] / (192 * n),
                 excluded_rgb_max=float(d_rgb[ex].max()) if n_ex else 0.0,
                 other_rays_differing=int((d_rgb[~ex] != 0).sum()), other_rgb_max=float(d_rgb[~ex].max()),
                 other_depth_max=float((dep1 - dep0)[~ex].abs().max()),
                 occupied_coarse=s["grid"].occupied_fraction(""), occupied_fine=s["grid"].occupied_fraction("fine"))
    print(family, precision, stats)
    parity_record("occupancy_vs_plain_render", f"{family}/{precision}/N64_dilate1", stats)
    assert torch.isfinite(rgb1).all() and torch.isfinite(dep1).all()
    assert n_ex <= 0.02 * n
    assert _same_bits(rgb1[~ex], rgb0[~ex]) and _same_bits(dep1[~ex], dep0[~ex])
    assert evaluated[0] == int(s["keep_c"].sum())                      # the coarse list is the coarse mark
    if s["culled_coarse_positive"] == 0:                               # then t_sorted is the plain one, and so is the fine list
        assert evaluated[1] == int(s["keep_f"].sum())
    assert evaluated[1] <= 0.5 * 192 * n
    if family == "sharp":
        assert evaluated[0] <= 0.5 * 64 * n


# ---- 4. degenerate grids ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_all_occupied_and_all_empty_grids(amd, scene, precision):
    s = scene("sharp", precision)
    net, o, d, n = s["net"], s["o"], s["d"], N_PROBE
    ones = torch.ones(5, 6, 7, device="cuda")
    full = amd.OccupancyGrid.from_fields(BIG_BOX, coarse=ones, fine=ones)
    empty = amd.OccupancyGrid.from_fields(BIG_BOX, coarse=-ones, fine=-ones)
    assert full.occupied_fraction("") == full.occupied_fraction("fine") == 1.0 and empty.occupied_fraction("fine") == 0.0
    rgb0, dep0, _ = s["plain"]
    rgb, dep, ev = _render(amd, net, o, d, full)
    assert _same_bits(rgb, rgb0) and _same_bits(dep, dep0) and ev == [64 * n, 192 * n]
    # with fast_sampling: the sampler's mask alone decides
    rgb_fs, dep_fs, _ = _render(amd, net, o, d, fast=True, threshold=0.02)
    rgb, dep, ev = _render(amd, net, o, d, full, fast=True, threshold=0.02)
    assert _same_bits(rgb, rgb_fs) and _same_bits(dep, dep_fs)
    assert ev[0] == 64 * n and 0 < ev[1] < 192 * n                     # the mask drops some
    # nothing evaluated: the white background, depth 0
    rgb, dep, ev = _render(amd, net, o, d, empty)
    assert (rgb == 1.0).all() and (dep == 0.0).all() and ev == [0, 0]
    rgb, dep, ev = _render(amd, net, o, d, empty, fast=True, threshold=0.02)
    assert (rgb == 1.0).all() and (dep == 0.0).all() and ev == [0, 0]
    # coarse only
    rgb_c, dep_c, _ = _render(amd, net, o, d, n_importance=0)
    rgb, dep, ev = _render(amd, net, o, d, full, n_importance=0)
    assert _same_bits(rgb, rgb_c) and _same_bits(dep, dep_c) and ev == [64 * n, 0]
    rgb, dep, ev = _render(amd, net, o, d, empty, n_importance=0)
    assert (rgb == 1.0).all() and (dep == 0.0).all() and ev == [0, 0]
    # one bitfield only: the other pass runs on every sample
    rgb, dep, ev = _render(amd, net, o, d, amd.OccupancyGrid.from_fields(BIG_BOX, fine=ones))
    assert _same_bits(rgb, rgb0) and _same_bits(dep, dep0) and ev == [64 * n, 192 * n]


# ---- 5. fast_sampling + occupancy ---------------------------------------------------------------------------------------------------
def test_fast_sampling_with_a_grid(amd, scene):
    s = scene("trained", "f32")
    ex = s["excluded"]
    rgb0, dep0, _ = _render(amd, s["net"], s["o"], s["d"], fast=True, threshold=0.02)
    rgb1, dep1, ev = _render(amd, s["net"], s["o"], s["d"], s["grid"], fast=True, threshold=0.02)
    assert _same_bits(rgb1[~ex], rgb0[~ex]) and _same_bits(dep1[~ex], dep0[~ex])
    assert ev[1] <= s["culled"][2][1]                                  # the mask AND the lookup: never more than the lookup alone


# ---- 6. ray blocks ------------------------------------------------------------------------------------------------------------------
def test_ray_blocks_change_nothing(amd, scene, monkeypatch):
    """200 rays in blocks of 64 (the last one of 8): the same bits as in one block, and `evaluated` sums over the blocks."""
    s = scene("sharp", "f32")
    o, d = s["o"][:200].contiguous(), s["d"][:200].contiguous()
    for kw in (dict(), dict(fast=True, threshold=0.02), dict(n_importance=0)):
        rgb0, dep0, ev0 = _render(amd, s["net"], o, d, s["grid"], **kw)
        monkeypatch.setenv("NERF_RENDER_BLOCK_RAYS", "64")
        rgb1, dep1, ev1 = _render(amd, s["net"], o, d, s["grid"], **kw)
        monkeypatch.delenv("NERF_RENDER_BLOCK_RAYS")
        assert _same_bits(rgb1, rgb0) and _same_bits(dep1, dep0) and ev1 == ev0
    rgb, dep, _ = _render(amd, s["net"], o, d, s["grid"])
    assert _same_bits(rgb, s["culled"][0][:200]) and _same_bits(dep, s["culled"][1][:200])       # rays are independent


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(amd, family_sd):
    o, d = (x[:64].contiguous() for x in _probe_rays())
    net = network(amd, family_sd("sharp"), "f32", train=False)
    grid = amd.OccupancyGrid.from_network(net, BOX, (9, 12, 17))
    r = amd.Renderer(net)
    r.occupancy = grid
    batch = {"rays_o": o[None], "rays_d": d[None]}
    with torch.no_grad():
        rgb, _ = r.render(batch)                                       # the grid is fine as long as nothing below applies
    assert torch.isfinite(rgb).all() and r.occupancy_stats is None

    def refused(exc, renderer=r, b=batch):
        with pytest.raises(exc) as info:
            renderer.render(b)
        return str(info.value)

    net.train()
    with torch.enable_grad():
        refused(NotImplementedError)
    net.eval()
    with torch.enable_grad():
        refused(NotImplementedError, b={"rays_o": o[None].clone().requires_grad_(True), "rays_d": d[None]})
    r.task = "train"
    with torch.no_grad():
        refused(NotImplementedError)
    r.task = "test"
    for precision in ("f16", "f16m32"):
        net.precision = precision
        with torch.no_grad():
            refused(NotImplementedError)
    net.precision = "f32"
    r.occupancy = "grid"
    with torch.no_grad():
        refused(TypeError)
    r.occupancy = grid
    # a stale grid: an in-place parameter update after from_network
    fields = amd.OccupancyGrid.from_fields(BOX, coarse=amd.density_grid(net, BOX, (9, 12, 17), model=""),
                                           fine=amd.density_grid(net, BOX, (9, 12, 17), model="fine"))
    assert torch.equal(fields.bits[""], grid.bits[""]) and torch.equal(fields.bits["fine"], grid.bits["fine"])
    with torch.no_grad():
        r.render(batch)
        net.model_fine.alpha_linear.bias.add_(0.0)
        assert "rebuild the grid" in refused(RuntimeError)
        r.N_importance = 0                                             # the coarse model did not change, and it alone is used
        r.render(batch)
        r.N_importance = 128
        r.occupancy = fields                                           # no key, no staleness check
        r.render(batch)
        r.occupancy = amd.OccupancyGrid.from_network(net, BOX, (9, 12, 17), models=("fine",))
        assert r.occupancy.bits[""] is None
        r.render(batch)
        net.model.alpha_linear.bias.add_(0.0)                          # not a model this grid was built from
        r.render(batch)
    torch.cuda.synchronize()
