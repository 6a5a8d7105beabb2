"""-m gpu: the geometry outputs -- nerf_density_gradient, nerf_composite_normals, Renderer.render_geometry, mesh.vertex_normals
(include/nerf_mi355x.h "geometry outputs").

The gradient is the data-gradient chain of the ray-gradient tests, so it is judged as tests/test_gpu_ray_grad.py judges it:
against float64, next to torch-fp32's own distance from float64, with that file's bars.  Everything that is a re-arrangement of
existing launches (blocking, positive_only, dead-tile skipping, the composed calls) is held to torch.equal.  The CPU references
(tests/normals_reference.py) are computed once per scene and shared."""
import pytest
import torch

import normals_reference as NR
from conftest import parity_record
from test_gpu_ray_grad import BARS          # f32 (3.0, 1e-3), f32x (4.0, 1e-3): the same chain, the project's bars
from gpu_common import amd, network  # noqa: F401

# Measured on the MI355X (profiles/parity_r03.json "gradients"): density_gradient/*, HIP q99 over torch-fp32 q99 of the per-point
# error: f32 1.40 (synthetic) / 1.09 (trained), f32x 0.94 / 1.05 -- q99 1.4e-6 .. 2.0e-6, every point within the bar;
# render_geometry_normal/trained: per-ray q99 4.6e-4 (f32) / 4.4e-4 (f32x) against torch-fp32's 4.3e-4; composite normals against
# float64: 1.9e-7 at most; the planar closed form: 3.3e-7 at most; vertex normals facing their faces: 0.9095, as with float64.

pytestmark = pytest.mark.gpu

ERR_WORKSPACE = -2


def _sd(scene, synthetic_sd, family_sd):
    return synthetic_sd if scene == "synthetic_sd" else family_sd("trained")


def _camera_rays(oracle, ids):
    return oracle.pinhole_rays(800, 800, oracle.camera_pose(30.0), pixel_ids=torch.as_tensor(ids))


def _jittered_t(n, S, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.linspace(2.0, 6.0, S)[None] + 0.01 * torch.rand(n, S, generator=gen)).contiguous()


def _density_gradient(amd, net, model, o, d, t, positive_only, block_points, stride=None, want_sigma=True):
    """nerf_density_gradient at the C ABI with a workspace of point_bytes * block_points -> (status, sigma [n,S], grad [n,S,3])."""
    lib, L = amd._lib.load(), amd._lib
    n, S = o.shape[0], t.shape[-1]
    sigma = torch.full((n, S), 7.0, device="cuda") if want_sigma else None
    grad = torch.full((n, S, 3), 7.0, device="cuda")
    ws = torch.empty(max(1, int(L.call("nerf_density_gradient_point_bytes")) * block_points), dtype=torch.uint8, device="cuda")
    rc = lib.nerf_density_gradient(L.ptr(o), L.ptr(d), L.ptr(t), S if stride is None else stride, n, S, net.packed(model).data_ptr(),
                                   net.packed_bwd(model).data_ptr(), int(positive_only), L.ptr(sigma), L.ptr(grad),
                                   L.PRECISIONS[net.precision], ws.data_ptr(), int(L.call("nerf_density_gradient_point_bytes")) * block_points,
                                   L.stream_of(o.device))
    torch.cuda.synchronize()
    return rc, sigma, grad


# ---- 1. the gradient at the ABI against float64 -----------------------------------------------------------------------------------
# five pixels of the oracle camera (theta 30) whose rays cross the object of the scene's fine model
OBJECT_PIXELS = {"synthetic_sd": (320000, 320640, 128400, 160400, 192400), "trained": (160400, 192400, 320640, 320680, 576400)}
_POINT_REFS = {}


def _point_refs(oracle, scene, sd):
    if scene not in _POINT_REFS:
        o, d = _camera_rays(oracle, OBJECT_PIXELS[scene])
        t = _jittered_t(5, 37, 9)
        pts = oracle.points_on_rays(o, d, t).reshape(-1, 3)                  # fp32, separately rounded: the kernels' points
        _POINT_REFS[scene] = (o, d, t, NR.sigma_and_gradient(sd, "model_fine", pts, torch.float32),
                              NR.sigma_and_gradient(sd, "model_fine", pts, torch.float64))
    return _POINT_REFS[scene]


@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("scene", ["synthetic_sd", "trained"])
def test_density_gradient_matches_float64(amd, oracle, synthetic_sd, family_sd, scene, precision):
    """5 rays x 37 samples = 185 points (a ragged last tile).  Per-point error |g - g64| / max(|g64|, 1e-3 max |g64|); at least 98 %
    of the points within FACTOR x torch-fp32's q99 + ABS (test_gpu_ray_grad._judge's rule and bars).  sigma is bit for bit the
    density-only forward's."""
    L = amd._lib
    sd = _sd(scene, synthetic_sd, family_sd)
    o, d, t, (_, g32), (s64, g64) = _point_refs(oracle, scene, sd)
    net = network(amd, sd, precision, train=False, frozen=True)
    oc, dc, tc = o.cuda(), d.cuda(), t.cuda()
    rc, sigma, grad = _density_gradient(amd, net, "fine", oc, dc, tc, 0, 192)       # 185 points, rounded up to whole tiles
    assert rc == 0
    raw = torch.empty(5, 37, 4, device="cuda")
    L.call("nerf_mlp_forward_rays_density", oc, dc, tc, 37, 5, 37, net.packed("fine"), raw, L.PRECISIONS[precision])
    assert torch.equal(sigma, raw[..., 3])
    assert (sigma.cpu().reshape(-1).double() - s64).abs().max() <= 1e-3 * max(1.0, s64.abs().max().item())
    assert (s64 > 0).any() and g64.abs().max() > 0
    norm64 = g64.norm(dim=-1)
    scale = norm64.clamp_min(1e-3 * norm64.max().item())
    e_hip = (grad.cpu().reshape(-1, 3).double() - g64).norm(dim=-1) / scale
    e_cpu = (g32.double() - g64).norm(dim=-1) / scale
    assert torch.isfinite(e_hip).all()
    q = lambda e: [torch.quantile(e, p).item() for p in (0.5, 0.9, 0.99, 1.0)]
    factor, abs_term = BARS[precision]
    bar = factor * q(e_cpu)[2] + abs_term
    within = (e_hip <= bar).float().mean().item()
    st = {"points": int(e_hip.numel()), "bar": bar, "share_within_bar": within, "hip_q50_q90_q99_max": q(e_hip),
          "torch_cpu_fp32_q50_q90_q99_max": q(e_cpu), "hip_over_torch_q99": q(e_hip)[2] / max(q(e_cpu)[2], 1e-30)}
    print(f"density gradient [{scene}/{precision}]: {st}")
    parity_record("gradients", f"density_gradient/{scene}/{precision}", st)
    assert within >= 0.98, st


# ---- 2. / 3. the composed calls, blocking, positive_only ---------------------------------------------------------------------------
# six rays of the trained checkpoint's fine model: 160400 / 192400 / 320640 / 320680 cross the object, 320200 / 320400 see nothing
# (sigma <= -2.5 on all 64 samples on the CPU), so whole 32-point tiles are dead
MIXED_PIXELS = (160400, 320200, 192400, 320400, 320640, 320680)


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_density_gradient_is_the_composed_calls_whatever_the_blocking(amd, oracle, family_sd, precision):
    lib, L = amd._lib.load(), amd._lib
    prec = L.PRECISIONS[precision]
    net = network(amd, family_sd("trained"), precision, train=False, frozen=True)
    o, d = (x.cuda() for x in _camera_rays(oracle, MIXED_PIXELS))
    n, S = 6, 64
    P = n * S
    t = _jittered_t(n, S, 10).cuda()
    st = L.stream_of(o.device)
    rc, sigma, grad = _density_gradient(amd, net, "fine", o, d, t, 0, P)
    assert rc == 0 and torch.isfinite(grad).all() and not (grad == 7.0).any()

    # 2. by hand: the density SAVE forward, the seed, the chain alone
    raw = torch.empty(P, 4, device="cuda")
    save = torch.empty(int(L.call("nerf_train_save_floats", P)), device="cuda")
    L.call("nerf_mlp_forward_rays_save_density", o, d, t, S, n, S, net.packed("fine"), raw, save, prec)
    assert torch.equal(sigma.reshape(-1), raw[:, 3])

    def by_hand(seed):
        draw = torch.zeros(P, 4, device="cuda")
        draw[:, 3] = seed
        gsave = torch.empty(int(L.call("nerf_train_grad_floats", P)), device="cuda")
        g_x = torch.full((P, 3), 7.0, device="cuda")
        L.call("nerf_mlp_backward_rays_x", o, d, t, S, n, S, net.packed_bwd("fine"), draw, save, gsave, None, g_x, None, 1, prec)
        torch.cuda.synchronize()
        return g_x.view(n, S, 3)
    assert torch.equal(grad, by_hand(1.0))
    positive = (raw[:, 3] > 0).float()
    rc, sigma_p, grad_p = _density_gradient(amd, net, "fine", o, d, t, 1, P)
    assert rc == 0 and torch.equal(sigma_p, sigma) and torch.equal(grad_p, by_hand(positive))

    # 3. positive_only: exactly zero where sigma <= 0, the full gradient elsewhere; some tiles dead, some live
    live = sigma > 0
    assert torch.all(grad_p[~live] == 0) and torch.equal(grad_p[live], grad[live]) and grad[~live].abs().max() > 0
    tiles = live.view(P // 32, 32).any(1)
    assert (~tiles).any() and tiles.any(), tiles.tolist()
    # blocking: all six rays, two rays (three blocks), one ray; a workspace below one ray is refused
    for positive_only, want in ((0, grad), (1, grad_p)):
        for rays in (2, 1):
            rc, s_b, g_b = _density_gradient(amd, net, "fine", o, d, t, positive_only, rays * S)
            assert rc == 0 and torch.equal(s_b, sigma) and torch.equal(g_b, want), (positive_only, rays)
    rc, _, g_b = _density_gradient(amd, net, "fine", o, d, t, 0, S - 1)
    assert rc == ERR_WORKSPACE and torch.all(g_b == 7.0)
    assert b"workspace" in lib.nerf_last_error()
    # sigma is optional; fp16 is refused; no rays is a no-op
    rc, _, g_b = _density_gradient(amd, net, "fine", o, d, t, 0, P, want_sigma=False)
    assert rc == 0 and torch.equal(g_b, grad)
    ws = torch.empty(int(L.call("nerf_density_gradient_point_bytes")) * P, dtype=torch.uint8, device="cuda")
    args = lambda n_rays, p: (L.ptr(o), L.ptr(d), L.ptr(t), S, n_rays, S, net.packed("fine").data_ptr(), net.packed_bwd("fine").data_ptr(),
                              0, None, L.ptr(g_b), p, ws.data_ptr(), ws.numel(), st)
    assert lib.nerf_density_gradient(*args(n, L.PREC_F16)) == -4 and lib.nerf_density_gradient(*args(0, prec)) == 0


# ---- 4. nerf_composite_normals against the float64 restatement --------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 192, 50])
def test_composite_normals_against_float64(amd, S):
    """acc is bit for bit the left-to-right fp32 sum of nerf_composite's `weights` output (the order the kernel states: one walk
    over the samples, k = 0 .. S-1); normal is within 192 * 4 * 2^-23 of the float64 value (non-negative weights that sum to at
    most 1, a few ulp per term); two runs write the same bytes."""
    lib, L = amd._lib.load(), amd._lib
    n = 7
    gen = torch.Generator().manual_seed(100 + S)
    raw = torch.randn(n, S, 4, generator=gen)
    raw[..., 3] = raw[..., 3] * 6.0 + 1.0                                   # about 43 % of the samples have sigma <= 0
    raw[3, :, 3] = -raw[3, :, 3].abs() - 0.1                                # an all-empty ray
    raw[5, : S // 2, 3] = -1.0                                              # a ray that is empty up to its middle
    grad = torch.randn(n, S, 3, generator=gen) * 10.0
    grad[:, 1::5] = 0.0                                                     # zero rows: no normal there
    grad[2, :, 1:] = 0.0                                                    # axis-aligned gradients
    t = _jittered_t(n, S, S)
    assert (raw[..., 3] <= 0).any() and (raw[..., 3] > 0).any()
    rawc, tc, gc = raw.cuda(), t.cuda(), grad.cuda()
    st = L.stream_of(rawc.device)

    def run():
        normal = torch.full((n, 3), 7.0, device="cuda")
        acc = torch.full((n,), 7.0, device="cuda")
        L.call("nerf_composite_normals", rawc, tc, S, n, S, gc, normal, acc)
        torch.cuda.synchronize()
        return normal, acc
    normal, acc = run()
    again = run()
    assert torch.equal(normal.view(torch.int32), again[0].view(torch.int32)) and torch.equal(acc.view(torch.int32), again[1].view(torch.int32))
    rgb, depth, weights = torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, S, device="cuda")
    L.call("nerf_composite", rawc, tc, S, n, S, 1, rgb, depth, weights)
    w = weights.cpu()
    acc_seq = torch.zeros(n)
    for k in range(S):
        acc_seq = acc_seq + w[:, k]                                         # fp32, left to right
    assert torch.equal(acc.cpu(), acc_seq)
    normal64, acc64, w64 = NR.composite_normals(raw, t, grad)
    assert (w.double() - w64).abs().max() <= 1e-5
    assert (acc.cpu().double() - acc64).abs().max() <= S * 2.0 ** -23
    err = (normal.cpu().double() - normal64).abs().max().item()
    print(f"composite normals S={S}: max|normal - float64| = {err:.3e}, max|acc - float64| = {(acc.cpu().double() - acc64).abs().max().item():.3e}")
    assert err <= 192 * 4 * 2.0 ** -23
    assert acc[3] == 0 and torch.all(normal[3] == 0) and acc64.max() > 0.9
    assert (normal.norm(dim=-1) <= acc * (1 + 1e-5) + 1e-6).all()           # not renormalised: |normal| <= acc
    # a shared depth table (stride 0) and the garbage a culled chain may leave where sigma <= 0 change nothing
    t0 = tc[0].contiguous()
    g_nan = torch.where((rawc[..., 3] <= 0)[..., None], torch.full_like(gc, float("nan")), gc)
    out = [torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda")]
    L.call("nerf_composite_normals", rawc, t0, 0, n, S, gc, out[0], out[1])
    L.call("nerf_composite_normals", rawc, t0, 0, n, S, g_nan, out[2], out[3])
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3]) and torch.equal(out[0][0], normal[0])
    assert lib.nerf_composite_normals(L.ptr(rawc), L.ptr(tc), 193, n, 193, L.ptr(gc), L.ptr(normal), L.ptr(acc), st) == -1


# ---- 5. closed form through the whole renderer ------------------------------------------------------------------------------------
# raw sigma(x) = a . x + c, a half-space: dyadic a; c puts the plane through the far end of the central ray of the oracle camera
# (theta 30), the camera on the empty side: of 64 random rays 34 end inside the half-space and 30 never enter it (CPU, margin 1e-3)
PLANE_A, PLANE_C = (2.0, -1.0, -4.0), -3.75


@pytest.mark.parametrize("n_importance", [128, 0])
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_planar_density_through_the_renderer(amd, oracle, synthetic_sd, precision, n_importance):
    sd = NR.planar_state_dict(synthetic_sd, PLANE_A, PLANE_C, "model_fine" if n_importance else "model")
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(5))[:64]
    o, d = _camera_rays(oracle, ids)
    a = torch.tensor(PLANE_A, dtype=torch.float64)
    s_near, s_far = (o + 2.0 * d).double() @ a + PLANE_C, (o + 6.0 * d).double() @ a + PLANE_C
    inside, never = s_far > 1e-3, (s_near < -1e-3) & (s_far < -1e-3)        # sigma is linear along a ray: its maximum is at an end
    assert inside.sum() >= 8 and never.sum() >= 8
    ren = amd.Renderer(network(amd, sd, precision, train=False, frozen=True))
    ren.N_importance = n_importance
    out = ren.render_geometry({"rays_o": o[None].cuda(), "rays_d": d[None].cuda()})
    normal, acc = out["normal"].cpu().double(), out["acc"].cpu().double()
    a_hat = a / a.norm()
    err = (normal + acc[:, None] * a_hat).abs().max().item()
    print(f"planar [{precision}, N_importance {n_importance}]: max|normal + acc a^| = {err:.3e}, acc on rays ending inside >= "
          f"{acc[inside].min().item():.6f}")
    assert err <= 1e-4
    assert (acc[inside] > 0.99).all()
    assert torch.all(out["acc"].cpu()[never] == 0) and torch.all(out["normal"].cpu()[never] == 0)
    rgb, depth = ren.render({"rays_o": o[None].cuda(), "rays_d": d[None].cuda()})
    assert torch.equal(out["rgb"], rgb) and torch.equal(out["depth"], depth)


# ---- 6. the render_geometry contract ----------------------------------------------------------------------------------------------
_FRAME_REFS = {}


def _frame_refs(oracle, sd):
    if not _FRAME_REFS:
        ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(8))[:96]
        o, d = _camera_rays(oracle, ids)
        _FRAME_REFS.update(o=o, d=d, fp32=NR.geometry_pipeline(sd, o, d, torch.float32), fp64=NR.geometry_pipeline(sd, o, d, torch.float64))
    return _FRAME_REFS


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_render_geometry_contract(amd, oracle, family_sd, monkeypatch, precision):
    """96 rays of the trained checkpoint in blocks of 40 (three blocks, one ragged): rgb / depth are render()'s, normal / acc do not
    depend on the blocking or on dead-tile skipping; the normal is judged against the float64 pipeline next to the torch-fp32
    pipeline's own distance from it, on the rays whose fp32 and float64 samplers pick the same bins: per-ray max |normal -
    normal64| <= FACTOR x torch-fp32's q99 + ABS on at least 98 % of them -- the rule and bars of the gradient the normal is made
    of (|normal| <= 1, so the absolute term is 1e-3 of the scale)."""
    sd = family_sd("trained")
    ref = _frame_refs(oracle, sd)
    batch = {"rays_o": ref["o"][None].cuda(), "rays_d": ref["d"][None].cuda()}
    ren = amd.Renderer(network(amd, sd, precision, train=False, frozen=True))
    rgb, depth = ren.render(batch)
    ren.geometry_block_rays = 40
    with torch.enable_grad():
        out = ren.render_geometry(batch)
    assert set(out) == {"rgb", "depth", "acc", "normal"} and not any(v.requires_grad for v in out.values())
    assert out["rgb"].shape == (96, 3) and out["depth"].shape == (96,) and out["acc"].shape == (96,) and out["normal"].shape == (96, 3)
    assert torch.equal(out["rgb"], rgb) and torch.equal(out["depth"], depth)
    ren.geometry_block_rays = 4096
    one = ren.render_geometry(batch)
    assert all(torch.equal(out[k], one[k]) for k in out)
    for env in ("0", "1"):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        ren.geometry_block_rays = 40
        other = ren.render_geometry(batch)
        assert all(torch.equal(out[k], other[k]) for k in out), env
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")
    ren.white_bkgd = False
    black = ren.render_geometry(batch)
    assert torch.equal(black["acc"], out["acc"]) and torch.equal(black["normal"], out["normal"]) and not torch.equal(black["rgb"], rgb)
    ren.white_bkgd = True

    f32, f64 = ref["fp32"], ref["fp64"]
    same = ((f32["bins"][0] == f64["bins"][0]) & (f32["bins"][1] == f64["bins"][1])).all(1)
    e_hip = (out["normal"].cpu().double() - f64["normal"]).abs().amax(1)
    e_cpu = (f32["normal"] - f64["normal"]).abs().amax(1)
    q = lambda e: [torch.quantile(e, p).item() for p in (0.5, 0.9, 0.99, 1.0)]
    factor, abs_term = BARS[precision]
    bar = factor * q(e_cpu[same])[2] + abs_term
    within = (e_hip[same] <= bar).float().mean().item()
    acc_err = (out["acc"].cpu().double() - f64["acc"]).abs()[same].max().item()
    st = {"rays": 96, "same_bins_in_fp64": int(same.sum()), "rays_with_acc_above_half": int((f64["acc"] > 0.5).sum()), "bar": bar,
          "share_within_bar": within, "hip_q50_q90_q99_max": q(e_hip[same]), "torch_cpu_fp32_q50_q90_q99_max": q(e_cpu[same]),
          "max_acc_error": acc_err}
    print(f"render_geometry normal [{precision}]: {st}")
    parity_record("gradients", f"render_geometry_normal/trained/{precision}", st)
    assert same.float().mean().item() >= 0.5 and (f64["acc"] > 0.5).sum() >= 8, st
    assert within >= 0.98, st
    assert acc_err <= 1e-3, st


@pytest.mark.parametrize("case", ["f16", "f16m32", "fast_sampling", "occupancy", "train_perturb", "rays_require_grad"])
def test_render_geometry_refuses_what_is_not_built(amd, oracle, synthetic_sd, case):
    net = network(amd, synthetic_sd, case if case.startswith("f16") else "f32", train=False, frozen=True)
    ren = amd.Renderer(net)
    o, d = (x.cuda() for x in _camera_rays(oracle, OBJECT_PIXELS["synthetic_sd"]))
    words = {"f16": "f16", "f16m32": "f16m32", "fast_sampling": "fast_sampling", "occupancy": "occupancy", "train_perturb": "perturb",
             "rays_require_grad": "require grad"}
    if case == "fast_sampling":
        ren.fast_sampling = True
    if case == "occupancy":
        ren.occupancy = amd.OccupancyGrid.from_network(network(amd, synthetic_sd, "f32", train=False, frozen=True), [-2, -2, -2, 2, 2, 2], 8)
    if case == "train_perturb":
        ren.task, ren.perturb = "train", True
    if case == "rays_require_grad":
        o = o.requires_grad_(True)
    launched = []
    ren._get_tables = lambda dev: launched.append(dev)                      # the first thing a permitted call does
    for grad_mode in (torch.no_grad, torch.enable_grad):
        with grad_mode(), pytest.raises(NotImplementedError, match=words[case]):
            ren.render_geometry({"rays_o": o[None], "rays_d": d[None]})
    assert not launched


# ---- 7. vertex normals of an extracted mesh ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_vertex_normals_of_an_extracted_mesh(amd, synthetic_sd, tmp_path, precision):
    from nerf_replication_amd.mesh import grid_axes
    net = network(amd, synthetic_sd, precision, train=False, frozen=True)
    box, N = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], 24
    grid = amd.density_grid(net, box, N)
    level = 0.5 * (grid.median().item() + grid.max().item())
    _, origin, step = grid_axes(box, N)
    v, f = amd.isosurface(grid, level, origin, step)
    V = v.shape[0]
    assert V >= 100 and f.shape[0] >= 100
    nrm = amd.vertex_normals(net, v)
    assert nrm.shape == (V, 3) and nrm.dtype == torch.float32 and nrm.is_cuda
    length = nrm.norm(dim=-1)
    assert torch.all((length == 0) | ((length - 1).abs() <= 1e-6)) and (length > 0).float().mean() > 0.9
    # the normalised gradient of the ABI entry at the vertices (one-sample rays: o = vertex, d = (0, 0, 1), t = 0), whatever the blocks
    dz = torch.tensor([[0.0, 0.0, 1.0]], device="cuda").expand(V, 3).contiguous()
    rc, sigma, g = _density_gradient(amd, net, "fine", v.contiguous(), dz, torch.zeros(1, device="cuda"), 0, 1024, stride=0)
    assert rc == 0
    g = g.view(V, 3)
    gn = g.norm(dim=-1, keepdim=True)
    assert torch.equal(nrm, torch.where(gn > 0, -g / torch.where(gn > 0, gn, torch.ones_like(gn)), torch.zeros_like(g)))
    _, g_all = amd.density_gradient(net, v)
    assert torch.equal(g_all, g) and torch.equal(amd.density_gradient(net, v, block_points=100)[1], g)
    # sigma at the vertices is near the level (they sit on the linear interpolant of a coarse grid, not on the true surface)
    print(f"vertex normals [{precision}]: {V} vertices, {f.shape[0]} triangles, level {level:.3f}, sigma at the vertices "
          f"{sigma.min().item():.3f} .. {sigma.max().item():.3f}")

    def share_facing(normals):
        """share of the vertices whose normal has a positive dot product with the area-weighted mean normal of their faces"""
        vc, fc = v.cpu().double(), f.cpu().long()
        face_n = torch.linalg.cross(vc[fc[:, 1]] - vc[fc[:, 0]], vc[fc[:, 2]] - vc[fc[:, 0]])       # length = 2 x area
        mean_n = torch.zeros(V, 3, dtype=torch.float64)
        for c in range(3):
            mean_n.index_add_(0, fc[:, c], face_n)
        return ((normals.cpu().double() * mean_n).sum(-1) > 0).double().mean().item()
    _, g64 = NR.sigma_and_gradient(synthetic_sd, "model_fine", v.cpu(), torch.float64)
    share, share64 = share_facing(nrm), share_facing(-g64)
    print(f"vertex normals [{precision}]: share facing their faces {share:.4f}, with float64 autograd gradients {share64:.4f}")
    parity_record("gradients", f"vertex_normals/synthetic/{precision}", {"vertices": V, "triangles": int(f.shape[0]),
                                                                          "share_facing_faces": share, "share_facing_faces_float64": share64})
    assert share >= share64 - 0.02
    # through extract_mesh into the file
    path = tmp_path / "mesh.ply"
    v1, f1 = amd.extract_mesh(net, level, box, str(path), N, normals=True)
    assert torch.equal(v1, v) and torch.equal(f1, f)
    names, rows, faces = NR.parse_ply(path.read_bytes())
    assert names == ["x", "y", "z", "nx", "ny", "nz"] and rows.shape == (V, 6)
    assert torch.equal(torch.from_numpy(rows[:, 3:].copy()), nrm.cpu()) and torch.equal(torch.from_numpy(rows[:, :3].copy()), v.cpu())
