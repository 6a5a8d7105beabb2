"""GPU tests of the hash field's spatial adjoint: every new entry alone, bit for bit against the fp32
restatement (tests/hashfield_grad_reference.py) inside guarded buffers, then HashField.density_gradient / vertex_normals /
vertex_colors, HashRenderer.render_geometry, the ray gradients and extract_mesh(field) against the float64 restatement under the
project's parity rule, per tensor

    max|hip - f64| <= 3 * max|cpu_fp32 - f64| + 2 u max|f64|,   u = 2^-24.

Measured / allowed go to profiles/hashfield_grad_parity.json.  Before anything is compared the restatement itself is asked whether the
comparison is decided: no hidden pre-activation (or density) of a compared row within the allowance of zero, no grid value within the
allowance of the level, no gradient of a sample with sigma > 0 below 1e-3 of the median."""
import functools

import numpy as np
import pytest
import torch

import hashfield_grad_reference as G
import hashfield_reference as R
import occupancy_reference as O
from test_gpu_hashfield import (GRID_N, PARAM_KEYS, Guarded, _allowed, batch_of, half_field, half_grid_words, hand_grid, hip_field,
                                hip_renderer, same)
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

U = R.U


def decided(pres64, pres32, what):
    """No value of the float64 tensors lies within the parity allowance of zero: a ReLU (or the sign of a density) decides the same
    way in every arithmetic compared."""
    for i, (p64, p32) in enumerate(zip(pres64, pres32)):
        p64 = p64.detach().double()
        allowance = 3 * float((p32.detach().double() - p64).abs().max()) + 2 * U * float(p64.abs().max())
        margin = float(p64.abs().min())
        print(f"{what}[{i}]: nearest value to zero {margin:.3e}, allowance {allowance:.3e}")
        assert margin > allowance, (what, i)


def gradients_not_small(gnorm, sigma, what):
    """... among the samples whose normal is formed at all: sigma > 0 and g . g > 0.  (A sample clamped on all three axes -- every
    sample of make_rays' ray 1, which misses the box -- has a gradient of exactly zero in every arithmetic, and n_i = 0 by definition.)"""
    g = gnorm[(sigma > 0) & (gnorm > 0)]
    ratio = float(g.min() / g.median())
    print(f"{what}: smallest |grad| over the median, among sigma > 0: {ratio:.3e}")
    assert ratio >= 1e-3, what


# ---- the entries alone ---------------------------------------------------------------------------------------------------------------
def entry_rays(n, S):
    """make_rays (rays from outside the box: the clamp zeroes the near samples; ray 1 misses the box) with, from 4 rays on, ray 3
    meeting the face z = 1.5 exactly at its first depth t = 2."""
    o, d = R.make_rays(n, seed=n * 1000 + S)
    if n > 3:
        o[3], d[3] = torch.tensor([0.25, 0.5, 3.5]), torch.tensor([0.0, 0.0, -1.0])
    return o, d


def compacted(n, S, gen):
    """An ascending list: a random half of the points, then rays 0, n - 1 and n // 2 lose every row and ray 5 keeps one."""
    keep = torch.rand(n, S, generator=gen) > 0.5
    if n >= 7:
        keep[0] = keep[n - 1] = keep[n // 2] = False
        keep[5] = False
        keep[5, S // 2] = True
    if not keep.any():
        keep[0, 0] = True
    return torch.nonzero(keep.reshape(-1)).reshape(-1).to(torch.int32)


@pytest.mark.parametrize("S", [1, 3, 64, 192])
@pytest.mark.parametrize("n", [1, 65])
def test_entries_are_the_restatement(amd, n, S):
    call = amd._lib.call
    o, d = entry_rays(n, S)
    t = torch.linspace(R.T_NEAR, R.T_FAR, S)
    frame = R.box_frame(R.BBOX)
    box = (frame[0].tolist(), frame[1].tolist(), frame[2])
    og, dg, tg = o.cuda(), d.cuda(), t.cuda()
    P = n * S
    gen = torch.Generator().manual_seed(n * 7 + S)
    for index in (None, compacted(n, S, gen)):
        M = P if index is None else int(index.numel())
        ig = None if index is None else index.cuda()
        p, _ = G.world_points(o, d, t, S, index, M)
        if n > 3 and index is None:
            assert float(p[3 * S, 2]) == 1.5                          # the sample on the face
            assert float((p.abs() > 1.5).double().mean()) > 0.05       # and the clamp has work to do

        # the seed, from a list and from column 0 of a [M,16] block, both flags
        sigma = torch.randn(M, generator=gen)
        sigma[::5] = 0.0
        sigma[M // 2] = float("nan")
        geo = torch.randn(M, 16, generator=gen)
        geo[:, 0] = sigma
        for positive_only in (0, 1):
            for src, stride in ((sigma, 1), (geo, 16)):
                out = Guarded((M, 16))
                call("nerf_field_density_seed", src.cuda(), stride, M, positive_only, out.view)
                assert same(out.view, G.seed(sigma, positive_only), "seed") and out.intact(), (positive_only, stride)

        # the rows, both layouts; the rays, with and without the view term and with one output alone
        g_x = torch.randn(M, 3, generator=gen)
        g_view = torch.randn(n, 3, generator=gen)
        want_p = G.points_backward(o, d, t, S, index, M, frame, g_x)
        want_o, want_d = G.ray_sums(o, d, t, S, index, M, frame, g_x)
        _, want_dv = G.ray_sums(o, d, t, S, index, M, frame, g_x, g_view)
        if n > 3 and index is None:
            assert float(want_p[3 * S, 2]) != 0 and float(want_p[S:2 * S].abs().sum()) == 0      # the face passes, ray 1 is clamped
        if index is not None and n >= 7:
            for r in (0, n - 1, n // 2):
                assert float(want_o[r].abs().sum()) == 0 and torch.equal(want_dv[r], g_view[r])
        gxg, gvg = g_x.cuda(), g_view.cuda()
        compact, full, g_o, g_d = Guarded((M, 3)), Guarded((P, 3), fill=7.0), Guarded((n, 3)), Guarded((n, 3))
        call("nerf_field_points_backward", og, dg, tg, 0, n, S, ig, M, *box, gxg, None, 0, compact.view, g_o.view, g_d.view)
        assert same(compact.view, want_p, "g_p") and compact.intact()
        assert same(g_o.view, want_o, "g_rays_o") and same(g_d.view, want_d, "g_rays_d") and g_o.intact() and g_d.intact()
        call("nerf_field_points_backward", og, dg, tg, 0, n, S, ig, M, *box, gxg, None, 1, full.view, None, None)
        assert same(full.view, G.by_id(want_p, index, M, P, 7.0), "g_p by id") and full.intact()
        g_d2, g_o2 = Guarded((n, 3)), Guarded((n, 3))
        call("nerf_field_points_backward", og, dg, tg, 0, n, S, ig, M, *box, gxg, gvg, 0, None, None, g_d2.view)
        assert same(g_d2.view, want_dv, "g_rays_d with the view term") and g_d2.intact()
        call("nerf_field_points_backward", og, dg, tg, 0, n, S, ig, M, *box, gxg, None, 0, None, g_o2.view, None)
        assert same(g_o2.view, want_o, "g_rays_o alone") and g_o2.intact()

        # the per-ray sums of the colour inputs' gradient
        g_cin = torch.randn(M, 32, generator=gen)
        g_sh = Guarded((n, 16))
        call("nerf_field_sh_gradient", g_cin.cuda(), ig, M, n, S, g_sh.view)
        want_sh = G.sh_gradient(g_cin, index, M, n, S)
        assert same(g_sh.view, want_sh, "g_sh") and g_sh.intact()
        if index is not None and n >= 7:
            assert float(want_sh[0].abs().sum()) == 0 and torch.equal(want_sh[5], g_cin[G.runs(index, M, n, S)[5][0], 16:])


@pytest.mark.parametrize("n", [1, 257])
def test_point_mode_backward(amd, n):
    frame = R.box_frame(R.BBOX)
    gen = torch.Generator().manual_seed(n)
    pts = (torch.rand(n, 3, generator=gen) - 0.5) * 4.0             # in [-2, 2]: some outside the box
    pts[0] = torch.tensor([1.5, -1.5, 0.0])                          # on two faces: passes
    if n > 2:
        pts[1] = torch.tensor([float("nan"), 0.0, 1.5000001])
    g_x = torch.randn(n, 3, generator=gen)
    out = Guarded((n, 3))
    amd._lib.call("nerf_field_points_backward", pts.cuda(), None, None, 0, n, 1, None, n, frame[0].tolist(), frame[1].tolist(), frame[2],
                  g_x.cuda(), None, 0, out.view, None, None)
    want = G.points_backward(pts, None, None, 1, None, n, frame, g_x)
    assert float(want[0].abs().min()) > 0 and (n <= 2 or torch.equal(want[1], torch.tensor([0.0, float(want[1, 1]), 0.0])))
    assert same(out.view, want, "g_p") and out.intact()


def test_sh4_encode_backward(amd):
    """Against float64 on the 1000 directions of the forward's test.  The unit of a row is 2^-23 max_k |g_sh[k]| / |d| (the fp32 ulp
    of 1.0 times the size of the row's incoming gradient and of the normalisation's factor); the allowance is the next integer above
    the distance of the fp32 restatement from float64 in that unit, measured on the CPU here."""
    from test_hashfield_grad_cpu import sh_test_directions
    d = sh_test_directions()
    g_sh = torch.randn(1000, 16, generator=torch.Generator().manual_seed(5))
    f32, f64 = G.sh4_backward(d, g_sh), G.sh4_backward(d, g_sh.double())
    unit = R.SH_ULP * g_sh.double().abs().max(dim=1).values / d.double().norm(dim=1)
    cpu_ulp = float(((f32.double() - f64).abs() / unit[:, None]).max())
    allowed = int(np.floor(cpu_ulp)) + 1
    out = Guarded((1000, 3))
    amd._lib.call("nerf_sh4_encode_backward", d.cuda(), g_sh.cuda(), 1000, out.view)
    hip_ulp = float(((out.view.cpu().double() - f64).abs() / unit[:, None]).max())
    print(f"fp32 restatement {cpu_ulp:.3f} ulp, device {hip_ulp:.3f} ulp, allowed {allowed}")
    G.parity_record("sh4_encode_backward", {"cpu_fp32_ulp": cpu_ulp, "hip_ulp": hip_ulp, "allowed_ulp": allowed})
    assert hip_ulp <= allowed and out.intact()
    assert same(out.view, f32, "g_rays_d_view")                   # and, like every glue entry, the fp32 restatement itself


# ---- density_gradient ----------------------------------------------------------------------------------------------------------------
def grid_points(N=16):
    from nerf_replication_amd.mesh import grid_axes
    axes, origin, step = grid_axes(R.BBOX, N)
    x, y, z = (torch.from_numpy(a.astype(np.float32)) for a in axes)
    return torch.stack(torch.meshgrid(x, y, z, indexing="ij"), dim=-1).reshape(-1, 3), origin, step


OUTSIDE = torch.tensor([[2.0, 0.1, 0.2], [0.3, -1.7, 9.0], [-3.0, -3.0, -3.0], [0.0, 0.0, 0.0]])


@functools.lru_cache(maxsize=None)
def density_reference(seed=9):
    sc = R.scene(65, 64, seed=seed)
    pts = torch.cat([grid_points()[0], OUTSIDE])
    out = {"scene": sc, "pts": pts}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        out[tag] = G.density_gradient(R.cast_params(sc["params"], dtype), pts, sc["frame"], sc["offsets"], sc["scales"], want_pres=True)
    return out


def test_density_gradient(amd):
    ref = density_reference()
    sc, pts = ref["scene"], ref["pts"]
    (s64, g64, pres64), (s32, g32, pres32) = ref["f64"], ref["cpu32"]
    decided(pres64 + [s64], pres32 + [s32], "density grid")
    field = hip_field(amd, sc, requires_grad=False)
    xyz = pts.cuda()
    sigma, grad = field.density_gradient(xyz)
    assert sigma.shape == (pts.shape[0],) and grad.shape == (pts.shape[0], 3) and not grad.requires_grad
    assert torch.equal(sigma, field.density(xyz)[:, 0])
    figures = {}
    ok = [_allowed("sigma", sigma, s64, s32, figures), _allowed("grad", grad, g64, g32, figures)]
    # outside the box: exact zeros on the clamped axes, a gradient on the others
    g_out = grad[-4:].cpu()
    assert float(g_out[0, 0]) == 0 and float(g_out[1, 1]) == 0 and float(g_out[1, 2]) == 0 and float(g_out[2].abs().sum()) == 0
    assert float(g_out[0, 1:].abs().min()) > 0 and float(g_out[3].abs().min()) > 0
    assert torch.equal(g_out == 0, g64[-4:] == 0)
    # positive_only: exactly zero where sigma <= 0, the same bytes elsewhere
    sigma_p, grad_p = field.density_gradient(xyz, positive_only=True)
    pos = sigma > 0
    assert 0.1 < float(pos.double().mean()) < 0.9
    assert torch.equal(sigma_p, sigma) and torch.equal(grad_p[pos], grad[pos]) and float(grad_p[~pos].abs().sum()) == 0
    # two runs write the same bytes
    again = field.density_gradient(xyz)
    assert torch.equal(again[0], sigma) and torch.equal(again[1], grad)
    # autograd through density(): positions and parameters both get gradients; the positions' is g * density_gradient
    field_t = hip_field(amd, sc, requires_grad=True)
    g = torch.randn(pts.shape[0], generator=torch.Generator().manual_seed(3))
    x = xyz.clone().requires_grad_(True)
    out = field_t.density(x)
    assert out.requires_grad and torch.equal(out.detach()[:, 0], sigma)
    (out[:, 0] * g.cuda()).sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in list(field_t.encoder.parameters()) + list(field_t.sigma_net.parameters()))
    ok.append(_allowed("density_backward_xyz", x.grad, g.double()[:, None] * g64, g[:, None] * g32, figures))
    G.parity_record("density_gradient_16", figures)
    assert all(ok), figures


# ---- render_geometry -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_reference(n, S, culled=False):
    sc = R.scene(n, S)
    keep = torch.from_numpy(O.keep(sc["o"].numpy(), sc["d"].numpy(), sc["t"].numpy(), *half_grid_words())) if culled else None
    out = {"scene": sc, "keep": keep}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        out[tag] = G.geometry(R.cast_params(sc["params"], dtype), sc["o"], sc["d"], sc["t"], sc["frame"], sc["offsets"], sc["scales"],
                              keep=keep, want_pres=True)
    return out


def _geometry_parity(amd, ref, ren, key):
    sc = ref["scene"]
    (acc64, nrm64, pres64, sig64, gn64), (acc32, nrm32, pres32, sig32, _) = ref["f64"], ref["cpu32"]
    decided(pres64 + [sig64], pres32 + [sig32], key)
    gradients_not_small(gn64, sig64, key)
    assert float(acc64.max()) > 0.5 and float(nrm64.abs().max()) > 0.05         # something is seen, and it has a direction
    rgb, depth, acc, normal = ren.render_geometry(batch_of(sc))
    n = sc["o"].shape[0]
    assert acc.shape == (n,) and normal.shape == (n, 3) and not normal.requires_grad
    stats, ren.stats = ren.stats, None
    plain = ren.render(batch_of(sc))
    ren.stats = stats
    assert torch.equal(rgb, plain[0]) and torch.equal(depth, plain[1])
    figures = {}
    ok = [_allowed("acc", acc, acc64, acc32, figures), _allowed("normal", normal, nrm64, nrm32, figures)]
    G.parity_record(key, figures)
    assert all(ok), figures
    return rgb, depth, acc, normal


@pytest.mark.parametrize("S", [3, 64, 192])
def test_render_geometry_parity(amd, S):
    ref = geometry_reference(65, S)
    ren = hip_renderer(amd, hip_field(amd, ref["scene"]), S, 1)    # parameters that require grad: the result is detached all the same
    _geometry_parity(amd, ref, ren, f"render_geometry_S{S}")
    with pytest.raises(NotImplementedError):
        ren.render_geometry({"rays_o": ref["scene"]["o"].cuda()[None].requires_grad_(True), "rays_d": ref["scene"]["d"].cuda()[None]})


def test_render_geometry_culled(amd):
    ref = geometry_reference(65, 64, culled=True)
    keep = ref["keep"]
    sc = ref["scene"]
    ren = hip_renderer(amd, hip_field(amd, sc, requires_grad=False), 64, 1)
    ren.occupancy, ren.stats = hand_grid(amd, half_field()), []
    _geometry_parity(amd, ref, ren, "render_geometry_half_box_S64")
    assert ren.stats == [(int(keep.sum()), 65 * 64)]
    # an all-negative grid: nothing is evaluated, nothing is seen
    ren.occupancy, ren.stats = hand_grid(amd, -np.ones((GRID_N,) * 3, dtype=np.float32)), []
    rgb, depth, acc, normal = ren.render_geometry(batch_of(sc))
    assert ren.stats == [(0, 65 * 64)]
    assert torch.equal(acc, torch.zeros(65, device="cuda")) and torch.equal(normal, torch.zeros(65, 3, device="cuda"))
    assert torch.equal(rgb, torch.ones(65, 3, device="cuda")) and torch.equal(depth, torch.zeros(65, device="cuda"))


def test_render_geometry_chunking_does_not_change_the_bytes(amd):
    sc = R.scene(100, 64)
    ren = hip_renderer(amd, hip_field(amd, sc, requires_grad=False), 64)
    results = []
    for chunk in (100, 33, 1):
        ren.geometry_chunk_rays = chunk
        results.append(ren.render_geometry(batch_of(sc)))
    for out in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out, results[0]))
    assert results[0][3].shape == (100, 3) and float(results[0][2].max()) > 0


# ---- ray gradients -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ray_reference(n, S, culled):
    sc = R.scene(n, S)
    keep = torch.from_numpy(O.keep(sc["o"].numpy(), sc["d"].numpy(), sc["t"].numpy(), *half_grid_words())) if culled else None
    gen = torch.Generator().manual_seed(77)
    a, b = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)
    out = {"scene": sc, "keep": keep, "a": a, "b": b}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        params = R.cast_params(sc["params"], dtype, requires_grad=True)
        od, dd = sc["o"].to(dtype).clone().requires_grad_(True), sc["d"].to(dtype).clone().requires_grad_(True)    # (copies: .to may alias)
        rgb, depth = G.render_rays(params, sc["o"], sc["d"], od, dd, sc["t"], sc["frame"], 1, sc["offsets"], sc["scales"], keep=keep)
        ((rgb * a.to(dtype)).sum() + (depth * b.to(dtype)).sum()).backward()
        _, pres = R.render(R.cast_params(sc["params"], dtype), sc["o"], sc["d"], sc["t"], sc["frame"], 1, sc["offsets"], sc["scales"],
                           keep=keep, want_pres=True)
        out[tag] = (rgb.detach(), depth.detach(), od.grad, dd.grad, [p.grad for p in R.flat_params(params)], pres)
    return out


@pytest.mark.parametrize("culled", [False, True])
@pytest.mark.parametrize("S", [3, 64])
def test_ray_gradients(amd, S, culled):
    ref = ray_reference(65, S, culled)
    sc = ref["scene"]
    r64, r32 = ref["f64"], ref["cpu32"]
    decided(r64[5], r32[5], f"rays S{S} culled{int(culled)}")
    assert float(r64[2].abs().max()) > 0 and float(r64[3].abs().max()) > 0
    field = hip_field(amd, sc)
    ren = hip_renderer(amd, field, S, 1)
    if culled:
        ren.occupancy = hand_grid(amd, half_field())
    with torch.no_grad():
        plain = ren.render(batch_of(sc))
    o, d = sc["o"].cuda()[None].requires_grad_(True), sc["d"].cuda()[None].requires_grad_(True)
    with pytest.raises(NotImplementedError):                       # the flag is opt-in: the refusal stands without it
        ren.render({"rays_o": o, "rays_d": d})
    ren.ray_gradients = True
    rgb, depth = ren.render({"rays_o": o, "rays_d": d})
    assert rgb.requires_grad and torch.equal(rgb.detach(), plain[0]) and torch.equal(depth.detach(), plain[1])
    flag_on_plain = ren.render(batch_of(sc))                        # rays that need no gradient: the flag changes nothing
    assert torch.equal(flag_on_plain[0].detach(), plain[0])
    ((rgb * ref["a"].cuda()).sum() + (depth * ref["b"].cuda()).sum()).backward()
    figures = {}
    ok = [_allowed("g_rays_o", o.grad[0], r64[2], r32[2], figures), _allowed("g_rays_d", d.grad[0], r64[3], r32[3], figures)]
    for name, p, g64, g32 in zip(PARAM_KEYS, field.parameters(), r64[4], r32[4]):
        assert p.grad is not None and float(g64.abs().max()) > 0, name
        ok.append(_allowed("grad_" + name, p.grad, g64, g32, figures))
    # a frozen field: the rays alone get gradients, the same ones under the rule
    frozen = hip_renderer(amd, hip_field(amd, sc, requires_grad=False), S, 1)
    frozen.occupancy, frozen.ray_gradients = ren.occupancy, True
    o2, d2 = sc["o"].cuda()[None].requires_grad_(True), sc["d"].cuda()[None].requires_grad_(True)
    rgb2, depth2 = frozen.render({"rays_o": o2, "rays_d": d2})
    ((rgb2 * ref["a"].cuda()).sum() + (depth2 * ref["b"].cuda()).sum()).backward()
    assert torch.equal(rgb2.detach(), plain[0]) and all(p.grad is None for p in frozen.field.parameters())
    ok += [_allowed("frozen_g_rays_o", o2.grad[0], r64[2], r32[2], figures), _allowed("frozen_g_rays_d", d2.grad[0], r64[3], r32[3], figures)]
    G.parity_record(f"ray_gradients_S{S}_culled{int(culled)}", figures)
    assert all(ok), [k for k, v in zip(figures, ok) if not v]


# ---- extract_mesh --------------------------------------------------------------------------------------------------------------------
def read_ply(path, n_v):
    """The vertex records of a PLY with x y z nx ny nz (float) and red green blue (uchar)."""
    data = open(path, "rb").read()
    head, _, body = data.partition(b"end_header\n")
    assert b"property float nx" in head and b"property uchar red" in head and f"element vertex {n_v}\n".encode() in head
    rec = np.frombuffer(body[:n_v * 27], dtype=np.dtype([("f", "<f4", (6,)), ("c", "u1", (3,))]))
    return rec["f"][:, 3:], rec["c"]


MESH_SEED = 8              # of R.scene.  With the default seed (9) one hidden pre-activation at one of the 12 506 vertices of the 16^3 mesh
# lies 2.7e-7 from zero, inside the allowance of 7.5e-7, so a ReLU could decide differently there.  Among the seeds 1..15, evaluated on
# the restatement at the vertices the device makes, 8 keeps the pre-activations farthest from zero (2.0e-6 against 5.6e-7) while no
# grid value is near the level (5.1e-5 against 3.6e-7); the test asserts both before it compares anything.


def test_extract_mesh_with_normals_and_colors(amd, tmp_path):
    from nerf_replication_amd.mesh import _head_on, isosurface
    N, level = 16, 0.0
    ref = density_reference(MESH_SEED)
    sc = ref["scene"]
    pts, origin, step = grid_points(N)
    params64, params32 = R.cast_params(sc["params"], torch.float64), R.cast_params(sc["params"], torch.float32)
    args = (sc["frame"], sc["offsets"], sc["scales"])
    g64, g32 = ref["f64"][0][:N ** 3], ref["cpu32"][0][:N ** 3]
    allowance = 3 * float((g32.double() - g64).abs().max()) + 2 * U * float(g64.abs().max())
    margin = float((g64 - level).abs().min())
    print(f"allowance {allowance:.3e}, nearest grid value to the level {margin:.3e}")
    assert margin > 2 * allowance

    field = hip_field(amd, sc, requires_grad=False)
    path = str(tmp_path / "field.ply")
    verts, faces = amd.extract_mesh(field, level, None, output_path=path, N=N, normals=True, colors=True)      # bbox: the field's own
    want_v, want_f = isosurface(g64.float().view(N, N, N).cuda(), level, origin, step)
    assert faces.shape[0] > 0 and torch.equal(faces, want_f) and verts.shape == want_v.shape
    with pytest.raises(TypeError):                                 # any other callable still cannot make normals
        amd.extract_mesh(field.density, level, R.BBOX, output_path=path + "x", N=N, normals=True)

    # the normals at the vertices the device made, against the restatement at the same fp32 positions
    v = verts.cpu()
    s64, gv64, pres64 = G.density_gradient(params64, v, *args, want_pres=True)
    s32, gv32, pres32 = G.density_gradient(params32, v, *args, want_pres=True)
    decided(pres64, pres32, "mesh vertices")
    gn = gv64.norm(dim=1)
    assert float(gn.min() / gn.median()) >= 1e-3
    normals = field.vertex_normals(verts)
    unit = lambda g: -g / g.norm(dim=1, keepdim=True)
    figures = {}
    ok = [_allowed("vertex_normals", normals, unit(gv64), unit(gv32), figures)]
    assert float((normals.norm(dim=1) - 1).abs().max()) <= 4 * U * 2
    # the colours for the device's own head-on directions (fp32), against the restatement with the same directions
    dirs = _head_on(normals)
    colors = field.vertex_colors(verts, dirs)
    assert torch.equal(colors, field.vertex_colors(verts))         # the default view direction is head-on
    x32 = R.points(v, None, None, 1, None, v.shape[0], sc["frame"])
    want = []
    for params in (params64, params32):
        rgb_raw, _, _ = R.field_rows(params, x32, R.sh4(dirs.cpu(), params["emb"].dtype), sc["offsets"], sc["scales"])
        want.append(torch.sigmoid(rgb_raw))
    ok.append(_allowed("vertex_colors", colors, want[0], want[1], figures))
    assert float(colors.min()) >= 0 and float(colors.max()) <= 1 and float(colors.std()) > 1e-3
    G.parity_record("extract_mesh_16", figures)
    assert all(ok), figures
    # the file holds exactly these normals and colours
    file_normals, file_colors = read_ply(path, v.shape[0])
    assert np.array_equal(file_normals, normals.cpu().numpy())
    assert np.array_equal(file_colors, np.floor(np.clip(colors.cpu().numpy().astype(np.float64), 0, 1) * 255 + 0.5).astype(np.uint8))
