"""CPU checks of the hash field's spatial adjoint: the restatement (tests/hashfield_grad_reference.py) against
torch autograd in float64 and against central differences, the third header against its binding table, the host refusals of the new
entries through the C ABI, and the Python refusals that happen before the library is reached."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hashfield_grad_reference as G
import hashfield_reference as R
import hashgrid_reference as H
from conftest import REPO
from test_fused_mlp_cpu import _declared_signatures, _declared_symbols

FIELD_HEADER = os.path.join(REPO, "include", "nerf_mi355x_field.h")
NEW_ENTRIES = ("nerf_field_density_seed", "nerf_field_points_backward", "nerf_field_sh_gradient", "nerf_sh4_encode_backward")


def sh_test_directions():
    """The 1000 directions of the forward's accuracy test (test_hashfield_cpu.sh_test_directions)."""
    gen = torch.Generator().manual_seed(11)
    d = torch.randn(1000, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    for i, axis in enumerate(torch.eye(3)):
        d[2 * i], d[2 * i + 1] = axis, -axis
    d[6] = d[6] * 1e-3
    return d


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_sh_adjoint_is_autograd_and_tangent():
    d = sh_test_directions()
    g_sh = torch.randn(1000, 16, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    dd = d.double().requires_grad_(True)
    (G.sh4_differentiable(dd) * g_sh).sum().backward()
    by_hand = G.sh4_backward(d, g_sh)
    scale = float(dd.grad.abs().max(dim=1).values.min())
    worst = float((by_hand - dd.grad).abs().max() / dd.grad.abs().max())
    print("max |by hand - autograd| relative", worst, "smallest row magnitude", scale)
    # (the normalisation is restated through float32's correctly rounded sqrt only in float32; in float64 it is exact to rounding)
    assert worst <= 1e-12
    radial = (by_hand * d.double()).sum(1).abs() / (by_hand.norm(dim=1) * d.double().norm(dim=1))
    print("max |g_d . d| / (|g_d| |d|)", float(radial.max()))
    assert float(radial.max()) <= 1e-13
    # the value path of sh4_differentiable is the header's basis
    assert float((G.sh4_differentiable(d.double()) - R.sh4(d, torch.float64)).abs().max()) <= 1e-14


def test_seed_and_points_backward_are_autograd():
    n, S = 7, 5
    o, d = R.make_rays(n, 1)
    t = torch.linspace(2.0, 6.0, S)
    frame = R.box_frame(R.BBOX)
    lo, hi, extent = frame
    assert torch.equal(G.seed(torch.tensor([1.0, 0.0, -2.0, float("nan")]), True)[:, 0], torch.tensor([1.0, 0.0, 0.0, 0.0]))
    assert torch.equal(G.seed(torch.tensor([1.0, 0.0, -2.0]), False)[:, 0], torch.ones(3)) and float(G.seed(torch.ones(3), True)[:, 1:].abs().sum()) == 0
    index = torch.tensor([0, 3, 4, 9, 21, 22, 34], dtype=torch.int32)
    M = index.numel()
    g_x = torch.randn(M, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    g_view = torch.randn(n, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    od, dd = o.double().requires_grad_(True), d.double().requires_grad_(True)
    ids = index.long()
    p = od[ids // S] + dd[ids // S] * t.double()[ids % S][:, None]
    x = (torch.clamp(p, min=lo.double(), max=hi.double()) - lo.double()) / extent
    ((x * g_x).sum() + (dd * g_view).sum()).backward()
    g_o, g_d = G.ray_sums(o, d, t, S, index, M, frame, g_x, g_view)
    assert float((g_o - od.grad).abs().max()) <= 1e-13 and float((g_d - dd.grad).abs().max()) <= 1e-12
    # ray 1 misses the box: every axis clamped, an exact zero; rays without rows (2, 3, 5) too
    g_p = G.points_backward(o, d, t, S, index, M, frame, g_x)
    assert torch.equal(g_p[3], torch.zeros(3, dtype=torch.float64)) and float(g_p.abs().sum()) > 0
    assert G.runs(index, M, n, S) == [(0, 3), (3, 4), (4, 4), (4, 4), (4, 6), (6, 6), (6, 7)]
    for r in (2, 3, 5):
        assert torch.equal(g_o[r], torch.zeros(3, dtype=torch.float64)) and torch.equal(g_d[r], g_view[r])
    # a sample exactly on a face passes (torch.clamp's rule), a NaN does not
    face = torch.tensor([[1.5, 0.0, -1.5], [1.5000001, 0.0, float("nan")]])
    g = G.points_backward(face, None, None, 1, None, 2, frame, torch.ones(2, 3))
    assert torch.equal(g, R.div_rn(torch.tensor([[1.0, 1.0, 1.0], [0.0, 1.0, 0.0]]), torch.full((2, 3), extent)))
    # the by-id layout leaves the other points alone
    full = G.by_id(g_p, index, M, n * S, 7.0)
    assert torch.equal(full[ids], g_p) and int((full == 7.0).all(dim=1).sum()) == n * S - M


def test_wave_sum_order():
    """Exact integers sum to the exact total whatever the order; the order itself shows on a cancelling triple."""
    v = torch.arange(1, 131, dtype=torch.float32)[:, None]
    assert float(G.wave_sum(v)) == 130 * 131 / 2 and float(G.wave_sum(v[:0])) == 0.0 and float(G.wave_sum(v[:1])) == 1.0
    # lanes 0 and 32 meet in the first fold step: (2^24 + 1) rounds to 2^24 before lane 1's -2^24 arrives
    w = torch.zeros(64, 1)
    w[0], w[32], w[16] = 2.0 ** 24, 1.0, -2.0 ** 24
    assert float(G.wave_sum(w)) == 0.0
    w[32], w[1] = 0.0, 1.0                                        # ... while lane 1 joins after the cancellation
    assert float(G.wave_sum(w)) == 1.0
    g_cin = torch.randn(9, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    index = torch.tensor([1, 2, 5, 6, 7, 8, 12, 13, 14], dtype=torch.int32)
    got = G.sh_gradient(g_cin, index, 9, 5, 3)
    want = torch.stack([g_cin[0:2, 16:].sum(0), g_cin[2:3, 16:].sum(0), g_cin[3:6, 16:].sum(0), torch.zeros(16, dtype=torch.float64),
                        g_cin[6:9, 16:].sum(0)])
    assert float((got - want).abs().max()) <= 1e-15 and torch.equal(got[3], torch.zeros(16, dtype=torch.float64))


def interior_points(sc, n, h):
    """World points inside the box whose normalised position stays, with a margin of 2 h, strictly inside one cell of every level."""
    lo, hi, extent = sc["frame"]
    gen = torch.Generator().manual_seed(4)
    xyz = (torch.rand(40 * n, 3, generator=gen) - 0.5) * 2.9
    x32 = R.points(xyz, None, None, 1, None, xyz.shape[0], sc["frame"])
    ok = torch.ones(xyz.shape[0], dtype=torch.bool)
    for s in sc["scales"]:
        _, f = H.cells(x32, s)
        ok &= ((f > 2 * h * float(s)) & (f < 1 - 2 * h * float(s))).all(dim=1)
    assert int(ok.sum()) >= n
    return xyz[ok][:n]


@pytest.mark.parametrize("positive_only", [False, True])
def test_density_gradient_by_hand_is_autograd_and_central_differences(positive_only):
    sc = R.scene(9, 5)
    h = 1e-6
    xyz = interior_points(sc, 64, h)
    args = (sc["frame"], sc["offsets"], sc["scales"])
    p64 = R.cast_params(sc["params"], torch.float64)
    sigma, grad = G.density_gradient(p64, xyz, *args, positive_only=positive_only)
    s_hand, g_hand = G.density_gradient_by_hand(sc["params"], xyz, *args, positive_only=positive_only)
    assert float((sigma - s_hand).abs().max()) <= 1e-12 and float((grad - g_hand).abs().max()) <= 1e-10
    assert 0 < int((sigma > 0).sum()) < 64 and float(grad.abs().max()) > 0
    if positive_only:
        assert float(grad[sigma <= 0].abs().max()) == 0
    # central differences in the normalised position, inside the cell and on one side of every ReLU
    x32 = R.points(xyz, None, None, 1, None, 64, sc["frame"])
    base, pres0 = G.sigma_of(p64, x32, x32.double(), sc["offsets"], sc["scales"])
    fd = torch.zeros(64, 3, dtype=torch.float64)
    same_side = torch.ones(64, dtype=torch.bool)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        up, pres_u = G.sigma_of(p64, x32, x32.double() + e, sc["offsets"], sc["scales"])
        dn, pres_d = G.sigma_of(p64, x32, x32.double() - e, sc["offsets"], sc["scales"])
        fd[:, a] = (up[:, 0] - dn[:, 0]) / (2 * h) / sc["frame"][2]
        for p0, pu, pd in zip(pres0, pres_u, pres_d):
            same_side &= ((p0 > 0) == (pu > 0)).all(dim=1) & ((p0 > 0) == (pd > 0)).all(dim=1)
    assert int(same_side.sum()) >= 60
    if positive_only:
        fd = fd * (sigma > 0)[:, None]
    err = float((fd - grad)[same_side].abs().max())
    print("max |central difference - gradient|", err, "of", float(grad.abs().max()))
    assert err <= 1e-6 * float(grad.abs().max())
    # outside the box the clamped axes are exact zeros
    out = torch.tensor([[2.0, 0.1, 0.2], [0.3, -1.7, 9.0]])
    _, g_out = G.density_gradient(p64, out, *args)
    assert float(g_out[0, 0]) == 0 and float(g_out[1, 1]) == 0 and float(g_out[1, 2]) == 0 and float(g_out[0, 1:].abs().min()) > 0


def test_render_rays_has_renders_values_and_autograd_gradients():
    """render_rays is R.render in value; its ray gradients are those of the chain composed by hand from the glue restatements."""
    n, S = 9, 5
    sc = R.scene(n, S)
    gen = torch.Generator().manual_seed(1)
    keep = torch.rand(n, S, generator=gen) > 0.4
    a, b = torch.randn(n, 3, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
    args = (sc["t"], sc["frame"], 1, sc["offsets"], sc["scales"])
    p64 = R.cast_params(sc["params"], torch.float64)
    od, dd = sc["o"].double().requires_grad_(True), sc["d"].double().requires_grad_(True)
    rgb, depth = G.render_rays(p64, sc["o"], sc["d"], od, dd, *args, keep=keep)
    want = R.render(p64, sc["o"], sc["d"], *args, keep=keep)
    assert torch.equal(rgb.detach(), want[0]) and torch.equal(depth.detach(), want[1])
    ((rgb * a).sum() + (depth * b).sum()).backward()
    # by hand: the gradients at (x, sh) by autograd through the rows, then the glue adjoints
    index = torch.nonzero(keep.reshape(-1)).reshape(-1).to(torch.int32)
    M = index.numel()
    ids = index.long()
    x32 = R.points(sc["o"], sc["d"], sc["t"], S, index, M, sc["frame"])
    xd = x32.double().requires_grad_(True)
    sh = R.sh4(sc["d"], torch.float64).requires_grad_(True)
    geo, _ = G.sigma_of(p64, x32, xd, sc["offsets"], sc["scales"])
    cin = torch.cat([geo, sh[ids // S]], dim=1)
    cin.retain_grad()
    rgb_raw, _ = R.mlp(cin, p64["cw"], p64["cb"])
    raw = R.raw_scatter(rgb_raw, geo[:, 0], index, M, n * S)
    r2, d2 = R.composite(raw.view(n, S, 4), sc["t"], 1, torch.float64)
    ((r2 * a).sum() + (d2 * b).sum()).backward()
    g_sh = G.sh_gradient(cin.grad, index, M, n, S)
    assert float((g_sh - sh.grad).abs().max()) <= 1e-12
    g_view = G.sh4_backward(sc["d"], g_sh)
    g_o, g_d = G.ray_sums(sc["o"], sc["d"], sc["t"], S, index, M, sc["frame"], xd.grad, g_view)
    print("max |by hand - autograd|", float((g_o - od.grad).abs().max()), float((g_d - dd.grad).abs().max()))
    assert float(od.grad.abs().max()) > 0 and float(dd.grad.abs().max()) > 0
    assert float((g_o - od.grad).abs().max()) <= 1e-10 * float(od.grad.abs().max())
    assert float((g_d - dd.grad).abs().max()) <= 1e-10 * float(dd.grad.abs().max())


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_field_header_declares_the_third_table():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(FIELD_HEADER)
    assert sorted(declared) == _declared_symbols(FIELD_HEADER) == sorted(L.FIELD_EXPORTS) == sorted(NEW_ENTRIES)
    assert tuple(L._FIELD_PROTOS) == L.FIELD_EXPORTS == tuple(L.FIELD_SIGNATURES)
    for name in NEW_ENTRIES:
        assert L.FIELD_SIGNATURES[name] == declared[name] and L.FIELD_SIGNATURES[name][0] == "status", name
    assert not set(L.FIELD_EXPORTS) & (set(L.EXPORTS) | set(L.NN_EXPORTS))
    assert len(L.EXPORTS) == 65 and len(L.NN_EXPORTS) == 11       # the two earlier tables do not move


def test_library_exports_the_new_entries():
    import nerf_replication_amd._lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert L.load().nerf_nn_abi_version() == 1 and L.load().nerf_abi_version() == 3


def test_entries_refuse_before_any_launch():
    """Host code: the pointers are never followed, so this runs without a GPU."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    p, odd = 0x10000, 0x10004
    box = (ctypes.c_float * 3)(0, 0, 0)

    def pb(o=p, d=p, t=p, stride=0, n=4, S=3, index=None, rows=5, lo=box, hi=box, extent=1.0, g_x=p, view=None, by_id=0, g_p=p,
           g_o=None, g_d=None):
        return lib.nerf_field_points_backward(o, d, t, stride, n, S, index, rows, lo, hi, extent, g_x, view, by_id, g_p, g_o, g_d, None)
    bad = [
        lib.nerf_field_density_seed(p, 1, 0, 0, p, None), lib.nerf_field_density_seed(None, 1, 5, 0, p, None),
        lib.nerf_field_density_seed(p, 1, 5, 0, None, None), lib.nerf_field_density_seed(p, 1, 5, 0, odd, None),
        lib.nerf_field_density_seed(p, 0, 5, 0, p, None), lib.nerf_field_density_seed(p, 1, 2 ** 31, 0, p, None),
        pb(rows=0), pb(rows=13), pb(S=0), pb(S=193), pb(n=0), pb(n=2 ** 31 // 192 + 1, S=192), pb(o=None), pb(g_x=None), pb(t=None),
        pb(stride=-1), pb(lo=None), pb(hi=None), pb(extent=0.0), pb(g_p=None),                      # no output at all
        pb(view=p),                                                                                  # the view term without g_rays_d
        pb(d=None), pb(d=None, S=1, n=5, g_o=p), pb(d=None, S=1, n=5, g_d=p), pb(d=None, S=1, n=5, g_p=None, g_d=p, view=p),
        lib.nerf_field_sh_gradient(p, None, 0, 4, 3, p, None), lib.nerf_field_sh_gradient(p, None, 13, 4, 3, p, None),
        lib.nerf_field_sh_gradient(p, None, 5, 4, 193, p, None), lib.nerf_field_sh_gradient(None, None, 5, 4, 3, p, None),
        lib.nerf_field_sh_gradient(p, None, 5, 4, 3, None, None), lib.nerf_field_sh_gradient(odd, None, 5, 4, 3, p, None),
        lib.nerf_field_sh_gradient(p, None, 5, 4, 3, odd, None),
        lib.nerf_sh4_encode_backward(p, p, 0, p, None), lib.nerf_sh4_encode_backward(None, p, 4, p, None),
        lib.nerf_sh4_encode_backward(p, None, 4, p, None), lib.nerf_sh4_encode_backward(p, p, 4, None, None),
        lib.nerf_sh4_encode_backward(p, odd, 4, p, None), lib.nerf_sh4_encode_backward(p, p, 2 ** 31, p, None),
    ]
    for rc in bad:
        assert rc == -1 and lib.nerf_last_error()


def small_field(pkg):
    enc = pkg.HashEncoder(input_dim=3, num_levels=4, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=12)
    return pkg.HashField(R.BBOX, encoder=enc)


def test_refusals_before_the_library(monkeypatch, tmp_path):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import _lib

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    field = small_field(pkg)
    renderer = pkg.HashRenderer(field)
    assert renderer.ray_gradients is False and renderer.geometry_chunk_rays == 4096
    rays = {"rays_o": torch.zeros(1, 4, 3), "rays_d": torch.ones(1, 4, 3)}
    grad_rays = {"rays_o": torch.zeros(1, 4, 3, requires_grad=True), "rays_d": torch.ones(1, 4, 3)}
    with pytest.raises(_lib.NerfLibraryError):                     # CPU tensors: no fallback
        renderer.render_geometry(rays)
    for flag in (False, True):                                     # render_geometry is inference only whatever the flag says
        renderer.ray_gradients = flag
        with pytest.raises(NotImplementedError):
            renderer.render_geometry(grad_rays)
    renderer.ray_gradients = False
    with pytest.raises(NotImplementedError):                       # the flag is opt-in
        renderer.render(grad_rays)
    renderer.ray_gradients = True
    with pytest.raises(_lib.NerfLibraryError):                     # with it, CPU rays are still refused
        renderer.render(grad_rays)
    for bad in (1, 0, None, "yes", 1.0):
        renderer.ray_gradients = bad
        with pytest.raises(ValueError, match="ray_gradients"):
            renderer.render(rays)
        with pytest.raises(ValueError, match="ray_gradients"):
            renderer.render_geometry(rays)
    renderer.ray_gradients = False
    for bad in (0, -1, 64.0, True, None, 8388607):
        renderer.geometry_chunk_rays = bad
        with pytest.raises(ValueError, match="geometry_chunk_rays"):
            renderer.render_geometry(rays)
    renderer.geometry_chunk_rays = 4096
    with pytest.raises(ValueError):
        renderer.render_geometry({"rays_o": torch.zeros(4, 3), "rays_d": torch.ones(4, 3)})
    half = small_field(pkg).half()
    with pytest.raises(NotImplementedError):                       # fp32 parameters only
        pkg.HashRenderer(half).render_geometry(rays)
    with pytest.raises(NotImplementedError):
        half.density_gradient(torch.zeros(5, 3))
    with pytest.raises(_lib.NerfLibraryError):
        field.density_gradient(torch.zeros(5, 3))
    with pytest.raises(_lib.NerfLibraryError):                     # positions that require grad go the same way: to a GPU or nowhere
        field.density(torch.zeros(5, 3, requires_grad=True))
    with pytest.raises(NotImplementedError):
        field.density_gradient(torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        field.density_gradient(torch.zeros(5, 2))
    with pytest.raises(_lib.NerfLibraryError):
        field.vertex_normals(torch.zeros(5, 3))
    with pytest.raises(_lib.NerfLibraryError):
        field.vertex_colors(torch.zeros(5, 3))
    with pytest.raises(ValueError):
        field.vertex_colors(torch.zeros(5, 3), viewdirs=torch.zeros(4, 3))
    with pytest.raises(ValueError):
        field.vertex_normals(torch.zeros(5, 2))
    # extract_mesh: a field is a queryfn with normals and colours; any other callable still is not
    with pytest.raises(TypeError, match="normals=True"):
        pkg.extract_mesh(lambda x: x, 0.0, R.BBOX, output_path=str(tmp_path / "a.ply"), N=4, normals=True)
    with pytest.raises(TypeError, match="colors=True"):
        pkg.extract_mesh(lambda x: x, 0.0, R.BBOX, output_path=str(tmp_path / "a.ply"), N=4, colors=True)
    with pytest.raises(ValueError, match="bbox is required"):
        pkg.extract_mesh(lambda x: x, 0.0, None, output_path=str(tmp_path / "a.ply"), N=4)
    with pytest.raises(_lib.NerfLibraryError):                     # a field on the CPU: its density refuses, bbox=None is its box
        pkg.extract_mesh(field, 0.0, None, output_path=str(tmp_path / "a.ply"), N=4, normals=True, colors=True)
    assert not os.path.exists(tmp_path / "a.ply")
