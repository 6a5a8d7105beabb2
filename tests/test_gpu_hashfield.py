"""GPU tests of the hash-grid radiance field: every glue entry bit for bit against the fp32 restatement
(tests/hashfield_reference.py) inside guarded buffers, then HashField / HashRenderer against the float64 restatement under the
project's parity rule (test_gpu_image_fit.py): per tensor

    max|hip - f64| <= 3 * max|cpu_fp32 - f64| + 2 u max|f64|,   u = 2^-24

with cpu_fp32 the same restatement in fp32 on the CPU.  Measured / allowed go to profiles/hashfield_parity.json."""
import functools

import numpy as np
import pytest
import torch

import hashfield_reference as R
import occupancy_reference as O
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

U = R.U
SENTINEL = -12345.5
PAD = 64                   # elements in front of and behind every guarded output (256 bytes: the views stay 16-byte aligned)


class Guarded:
    """An output inside a sentinel-filled buffer; intact() says whether everything around it still holds the sentinel."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.whole[PAD:PAD + n].view(shape)
        if fill is not None:
            self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        w = self.whole.cpu()
        return bool((w[:PAD] == SENTINEL).all() and (w[-PAD:] == SENTINEL).all())


def same(got, want, what=""):
    """Bit equality of a device result with the restatement; the elements that differ are printed with their bits."""
    got = got.detach().cpu()
    if torch.equal(got, want):
        return True
    bad = torch.nonzero(got != want)
    print(f"{what}: {bad.shape[0]} of {want.numel()} elements differ; the first ones (index, device, restatement, bits):")
    for idx in bad[:12].tolist():
        g, w = got[tuple(idx)], want[tuple(idx)]
        print("  ", idx, float(g), float(w), hex(g.view(torch.int32).item() & 0xffffffff), hex(w.view(torch.int32).item() & 0xffffffff))
    return False


def _allowed(name, hip, f64, cpu32, figures):
    """max|hip - f64| <= 3 max|cpu32 - f64| + 2 u max|f64|; both distances are kept."""
    f64 = f64.detach().double().cpu()
    d_hip = float((hip.detach().double().cpu() - f64).abs().max())
    d_cpu = float((cpu32.detach().double().cpu() - f64).abs().max())
    allowance = 3 * d_cpu + 2 * U * float(f64.abs().max())
    figures[name] = {"hip_vs_f64": d_hip, "cpu_fp32_vs_f64": d_cpu, "allowance": allowance}
    print(f"{name}: hip {d_hip:.3e} cpu fp32 {d_cpu:.3e} allowance {allowance:.3e}")
    return d_hip <= allowance


def hip_field(amd, sc, requires_grad=True):
    """The package's HashField holding a scene's parameters."""
    enc = amd.HashEncoder(input_dim=3, num_levels=sc["L"], level_dim=2, per_level_scale=2, base_resolution=16,
                          log2_hashmap_size=sc["T"])
    assert enc.offsets.tolist() == list(sc["offsets"])
    field = amd.HashField(R.BBOX, encoder=enc, width=sc["width"])
    with torch.no_grad():
        for p, v in zip(field.parameters(), R.flat_params(sc["params"])):
            assert p.shape == v.shape
            p.copy_(v)
    field = field.cuda()
    for p in field.parameters():
        p.requires_grad_(requires_grad)
    return field


def hip_renderer(amd, field, S, white=True):
    ren = amd.HashRenderer(field)
    ren.N_samples, ren.white_bkgd = S, bool(white)
    assert (ren.t_near, ren.t_far) == (R.T_NEAR, R.T_FAR)
    return ren


def batch_of(sc):
    return {"rays_o": sc["o"].cuda()[None], "rays_d": sc["d"].cuda()[None]}


PARAM_KEYS = ["encoder.embeddings"] + [f"sigma_net.layers.{i}.{p}" for i in range(2) for p in ("weight", "bias")] + \
             [f"color_net.layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")]


@functools.lru_cache(maxsize=None)
def reference(n, S, white, culled=False, with_grads=False):
    """The restatement of the parity scene in float64 and in fp32 on the CPU, computed once per case: {"scene", "keep", and per dtype
    (rgb, depth, [parameter gradients of sum(rgb a) + sum(depth b)])}."""
    sc = R.scene(n, S)
    keep = None
    if culled:
        keep = torch.from_numpy(O.keep(sc["o"].numpy(), sc["d"].numpy(), sc["t"].numpy(), *half_grid_words()))
    gen = torch.Generator().manual_seed(77)
    a, b = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)
    out = {"scene": sc, "keep": keep, "a": a, "b": b}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        params = R.cast_params(sc["params"], dtype, requires_grad=with_grads)
        (rgb, depth), pres = R.render(params, sc["o"], sc["d"], sc["t"], sc["frame"], white, sc["offsets"], sc["scales"], keep=keep,
                                      want_pres=True)
        out.setdefault("sigma_positive", float((pres[-1] > 0).double().mean()))
        grads = None
        if with_grads:
            ((rgb * a.to(dtype)).sum() + (depth * b.to(dtype)).sum()).backward()
            grads = [p.grad for p in R.flat_params(params)]
        out[tag] = (rgb.detach(), depth.detach(), grads)
    return out


# ---- the glue entries, bit for bit ---------------------------------------------------------------------------------------------------
def index_cases(P, seed):
    """None, and random ascending subsets with M in {1, 33, P} (those that fit)."""
    gen = torch.Generator().manual_seed(seed)
    cases = [(None, P)]
    for M in sorted({1, min(33, P), P}):
        ids = torch.sort(torch.randperm(P, generator=gen)[:M]).values.to(torch.int32)
        cases.append((ids, M))
    return cases


@pytest.mark.parametrize("S", [1, 3, 192])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_glue_entries_are_the_restatement(amd, n, S):
    """Rays start outside the box (the clamp works on the near samples), ray 0 looks along -z exactly, ray 1 misses the box."""
    call = amd._lib.call
    o, d = R.make_rays(n, seed=n * 1000 + S)
    t = torch.linspace(R.T_NEAR, R.T_FAR, S)
    frame = R.box_frame(R.BBOX)
    lo, hi, extent = frame[0].tolist(), frame[1].tolist(), frame[2]
    og, dg, tg = o.cuda(), d.cuda(), t.cuda()
    P = n * S
    gen = torch.Generator().manual_seed(n + S)
    if n > 1:                                                      # the clamp has work to do
        assert float((o[:, None, :] + d[:, None, :] * t[None, :, None]).abs().max()) > 1.5

    sh = Guarded((n, 16))
    call("nerf_sh4_encode", dg, n, sh.view)
    sh_ref = R.sh4(d)
    assert same(sh.view, sh_ref, "sh") and sh.intact()

    for index, M in index_cases(P, seed=n * S):
        ig = None if index is None else index.cuda()
        x = Guarded((M, 3))
        call("nerf_field_points", og, dg, tg, 0, n, S, ig, M, lo, hi, extent, x.view)
        want = R.points(o, d, t, S, index, M, frame)
        assert same(x.view, want, "x") and x.intact(), (index is None, M)

        geo = torch.randn(M, 16, generator=gen)
        cin, sig = Guarded((M, 32)), Guarded((M,))
        call("nerf_field_color_inputs", geo.cuda(), sh.view, ig, M, n, S, cin.view, sig.view)
        want_cin, want_sig = R.color_inputs(geo, sh_ref, S, index, M)
        assert same(cin.view, want_cin, "cin") and same(sig.view, want_sig, "sigma_rows") and cin.intact() and sig.intact()

        g_cin, g_sig = torch.randn(M, 32, generator=gen), torch.randn(M, generator=gen)
        g_geo = Guarded((M, 16))
        call("nerf_field_color_inputs_backward", g_cin.cuda(), g_sig.cuda(), M, g_geo.view)
        assert same(g_geo.view, R.color_inputs_backward(g_cin, g_sig), "g_geo") and g_geo.intact()

        rgb = torch.randn(M, 3, generator=gen)
        raw = Guarded((P, 4), fill=0.0)
        call("nerf_field_raw_scatter", rgb.cuda(), sig.view, ig, M, P, raw.view)
        assert same(raw.view, R.raw_scatter(rgb, want_sig, index, M, P), "raw") and raw.intact()

        g_raw = torch.randn(P, 4, generator=gen)
        g_rgb, g_s = Guarded((M, 3)), Guarded((M,))
        call("nerf_field_raw_gather", g_raw.cuda(), ig, M, P, g_rgb.view, g_s.view)
        want_rgb, want_s = R.raw_gather(g_raw, index, M)
        assert same(g_rgb.view, want_rgb, "g_rgb") and same(g_s.view, want_s, "g_sigma_rows") and g_rgb.intact() and g_s.intact()


@pytest.mark.parametrize("n", [1, 257])
def test_point_mode(amd, n):
    frame = R.box_frame(R.BBOX)
    pts = (torch.rand(n, 3, generator=torch.Generator().manual_seed(n)) - 0.5) * 4.0        # in [-2, 2]: some outside the box
    x = Guarded((n, 3))
    amd._lib.call("nerf_field_points", pts.cuda(), None, None, 0, n, 1, None, n, frame[0].tolist(), frame[1].tolist(), frame[2], x.view)
    assert same(x.view, R.points(pts, None, None, 1, None, n, frame), "x") and x.intact()


# ---- render and gradient parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [1, 0])
@pytest.mark.parametrize("S", [3, 64, 192])
def test_render_parity(amd, S, white):
    ref = reference(65, S, white)
    sc = ref["scene"]
    assert 0.3 < ref["sigma_positive"] < 0.7                       # about half of the samples have sigma > 0
    assert float(ref["f64"][0].std()) > 1e-3                       # the image is not flat
    ren = hip_renderer(amd, hip_field(amd, sc, requires_grad=False), S, white)
    rgb, depth = ren.render(batch_of(sc))
    assert rgb.shape == (65, 3) and depth.shape == (65,) and not rgb.requires_grad
    figures = {}
    ok = [_allowed("rgb", rgb, ref["f64"][0], ref["cpu32"][0], figures), _allowed("depth", depth, ref["f64"][1], ref["cpu32"][1], figures)]
    R.parity_record(f"render_S{S}_white{white}", figures)
    assert all(ok), figures
    with torch.no_grad():                                          # grad mode does not change the bytes
        again = ren.render(batch_of(sc))
    assert torch.equal(again[0], rgb) and torch.equal(again[1], depth)


def _gradient_parity(amd, ref, ren, key):
    sc = ref["scene"]
    field = ren.field
    rgb, depth = ren.render(batch_of(sc))
    assert rgb.requires_grad and depth.requires_grad
    ((rgb * ref["a"].cuda()).sum() + (depth * ref["b"].cuda()).sum()).backward()
    figures, ok = {}, []
    for name, p, g64, g32 in zip(PARAM_KEYS, field.parameters(), ref["f64"][2], ref["cpu32"][2]):
        assert p.grad is not None and p.grad.shape == g64.shape, name
        ok.append(_allowed("grad_" + name, p.grad, g64, g32, figures))
        assert float(g64.abs().max()) > 0, name
    # table rows no sample touches: exactly zero in float64, so exactly zero on the device
    g_emb, g64 = field.encoder.embeddings.grad.cpu(), ref["f64"][2][0]
    untouched = g64 == 0
    assert 0 < int(untouched.sum()) < untouched.numel()
    assert bool((g_emb[untouched] == 0).all())
    ok.append(_allowed("rgb", rgb, ref["f64"][0], ref["cpu32"][0], figures))
    R.parity_record(key, figures)
    assert all(ok), [k for k, o in zip(figures, ok) if not o]


def test_gradient_parity(amd):
    ref = reference(65, 64, 1, with_grads=True)
    ren = hip_renderer(amd, hip_field(amd, ref["scene"]), 64, 1)
    _gradient_parity(amd, ref, ren, "gradients_S64")


def test_chunking_does_not_change_the_bytes(amd):
    sc = R.scene(100, 64)
    ren = hip_renderer(amd, hip_field(amd, sc, requires_grad=False), 64)
    results = []
    for chunk in (100, 33, 1):
        ren.chunk_rays = chunk
        results.append(ren.render(batch_of(sc)))
    for rgb, depth in results[1:]:
        assert torch.equal(rgb, results[0][0]) and torch.equal(depth, results[0][1])
    assert results[0][0].shape == (100, 3)


# ---- culling, with hand-made grids ---------------------------------------------------------------------------------------------------
GRID_BBOX = (-16.0, -16.0, -16.0, 16.0, 16.0, 16.0)             # contains every sample of make_rays (ray 1 reaches x = 15)
GRID_N = 17                                                      # cells of 2 units; the plane x = 0 is a cell boundary


def half_field():
    f = -np.ones((GRID_N,) * 3, dtype=np.float32)
    f[:GRID_N // 2] = 1.0                                        # grid points with x < 0
    return f


@functools.lru_cache(maxsize=None)
def half_grid_words():
    """(words, dims, box_min, inv) of the half-box grid as occupancy_reference builds it: cells with a corner at x < 0."""
    dims = (GRID_N,) * 3
    return (O.build(half_field(), 0.0, 0), dims) + tuple(O.lookup_frame(GRID_BBOX, dims))


def hand_grid(amd, field_np):
    return amd.OccupancyGrid.from_fields(GRID_BBOX, fine=torch.from_numpy(field_np).cuda(), level=0.0, dilate=0)


@pytest.mark.parametrize("white", [1, 0])
def test_culling_all_and_nothing(amd, white):
    sc = R.scene(65, 64)
    ren = hip_renderer(amd, hip_field(amd, sc, requires_grad=False), 64, white)
    plain = ren.render(batch_of(sc))
    ren.occupancy, ren.stats = hand_grid(amd, np.ones((GRID_N,) * 3, dtype=np.float32)), []
    full = ren.render(batch_of(sc))
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1]) and ren.stats == [(65 * 64, 65 * 64)]
    ren.occupancy, ren.stats = hand_grid(amd, -np.ones((GRID_N,) * 3, dtype=np.float32)), []
    empty = ren.render(batch_of(sc))
    assert torch.equal(empty[0], torch.full((65, 3), float(white), device="cuda")) and torch.equal(empty[1], torch.zeros(65, device="cuda"))
    assert ren.stats == [(0, 65 * 64)]


def test_culling_half_box(amd):
    ref = reference(65, 64, 1, culled=True, with_grads=True)
    keep = ref["keep"]
    assert 0.2 < float(keep.double().mean()) < 0.8                 # the grid culls a real share
    ren = hip_renderer(amd, hip_field(amd, ref["scene"]), 64, 1)
    grid = hand_grid(amd, half_field())
    assert np.array_equal(grid.bits["fine"].cpu().numpy().view(np.uint32), half_grid_words()[0])
    ren.occupancy, ren.stats = grid, []
    _gradient_parity(amd, ref, ren, "culled_half_box_S64")
    assert ren.stats == [(int(keep.sum()), 65 * 64)]
    ren.chunk_rays, ren.stats = 20, []                             # per chunk, and the chunking does not move the image
    with torch.no_grad():
        rgb, _ = ren.render(batch_of(ref["scene"]))
    assert ren.stats == [(int(keep[i:i + 20].sum()), keep[i:i + 20].numel()) for i in range(0, 65, 20)]
    figures = {}
    assert _allowed("rgb", rgb, ref["f64"][0], ref["cpu32"][0], figures)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(amd):
    from nerf_replication_amd.occupancy import OccupancyGrid
    sc = R.scene(5, 3)
    field = hip_field(amd, sc)
    half = hip_field(amd, sc).half()
    ren, ren_half = hip_renderer(amd, field, 3), hip_renderer(amd, half, 3)
    o, d = sc["o"].cuda()[None], sc["d"].cuda()[None]
    cpu_grid = OccupancyGrid(np.array(GRID_BBOX).reshape(2, 3), (4, 4, 4), 0.0, 0, {"": None, "fine": torch.zeros(2, dtype=torch.int32)}, None)
    coarse_only = amd.OccupancyGrid.from_fields(GRID_BBOX, coarse=torch.ones(4, 4, 4, device="cuda"))
    torch.cuda.synchronize()

    def refused(exc, renderer, batch):
        before = torch.cuda.memory_allocated()
        with pytest.raises(exc):
            renderer.render(batch)
        assert torch.cuda.memory_allocated() == before
    refused(NotImplementedError, ren, {"rays_o": o.clone().requires_grad_(True), "rays_d": d})
    refused(NotImplementedError, ren, {"rays_o": o, "rays_d": d.clone().requires_grad_(True)})
    refused(NotImplementedError, ren_half, {"rays_o": o, "rays_d": d})
    refused(amd._lib.NerfLibraryError, ren, {"rays_o": o.cpu(), "rays_d": d.cpu()})
    ren.occupancy = cpu_grid
    refused(ValueError, ren, {"rays_o": o, "rays_d": d})
    ren.occupancy = coarse_only
    refused(ValueError, ren, {"rays_o": o, "rays_d": d})
    ren.occupancy = "grid"
    refused(TypeError, ren, {"rays_o": o, "rays_d": d})
    ren.occupancy = None
    ren.N_samples = 193
    refused(ValueError, ren, {"rays_o": o, "rays_d": d})
    ren.N_samples = 3
    # an empty batch: empty tensors, nothing launched or allocated beyond them
    rgb, depth = ren.render({"rays_o": o[:, :0], "rays_d": d[:, :0]})
    assert rgb.shape == (0, 3) and depth.shape == (0,) and rgb.is_cuda
    assert ren.render({"rays_o": o, "rays_d": d})[0].shape == (5, 3)


# ---- density, occupancy_grid, extract_mesh -------------------------------------------------------------------------------------------
def test_density_grid_and_mesh(amd, tmp_path):
    """The seed of R.scene is one for which no value of the 16^3 density grid lies within the parity allowance of the level: checked
    here on the restatement before anything is compared.  Then the inside / outside pattern of the device grid is the restatement's,
    extract_mesh(field.density) has the faces isosurface makes from the restatement's grid, and its vertices sit where those do up to
    the interpolation's sensitivity: a vertex is p0 + step (level - f0) / (f1 - f0), and errors of at most `a` in f0 and f1 move the
    fraction by at most 3 a / |f1 - f0| <= 1.5 a / margin, margin = min |f - level| (both ends are at least that far from it)."""
    from nerf_replication_amd.mesh import grid_axes, isosurface
    N, level = 16, 0.0
    sc = R.scene(65, 64)
    axes, origin, step = grid_axes(R.BBOX, N)
    x, y, z = (torch.from_numpy(a.astype(np.float32)) for a in axes)
    pts = torch.stack(torch.meshgrid(x, y, z, indexing="ij"), dim=-1).reshape(-1, 3)
    g64 = R.density(R.cast_params(sc["params"], torch.float64), pts, sc["frame"], sc["offsets"], sc["scales"])
    g32 = R.density(R.cast_params(sc["params"], torch.float32), pts, sc["frame"], sc["offsets"], sc["scales"])
    allowance = 3 * float((g32.double() - g64).abs().max()) + 2 * U * float(g64.abs().max())
    margin = float((g64 - level).abs().min())
    print(f"allowance {allowance:.3e}, nearest grid value to the level {margin:.3e}")
    assert margin > 2 * allowance
    assert 0.1 < float((g64 > level).double().mean()) < 0.9

    field = hip_field(amd, sc, requires_grad=False)
    sigma = field.density(pts.cuda())
    assert sigma.shape == (N ** 3, 1) and not sigma.requires_grad
    figures = {}
    assert _allowed("density_grid", sigma[:, 0], g64, g32, figures)
    R.parity_record("density_grid_16", figures)
    assert torch.equal(sigma[:, 0].cpu() > level, g64 > level)

    verts, faces = amd.extract_mesh(field.density, level, R.BBOX, output_path=str(tmp_path / "field.ply"), N=N)
    want_v, want_f = isosurface(g64.float().view(N, N, N).cuda(), level, origin, step)
    assert faces.shape[0] > 0 and torch.equal(faces, want_f) and verts.shape == want_v.shape
    tol = max(step) * 1.5 * allowance / margin + 8 * U * 1.5
    assert float((verts - want_v).abs().max()) <= tol

    grid = field.occupancy_grid(N=N, level=level, dilate=1)
    assert grid.bits[""] is None and grid.keys is None
    cells = O.cells(g64.float().view(N, N, N).numpy(), level, 1)
    assert np.array_equal(grid.cells("fine").cpu().numpy(), cells) and 0 < cells.mean()
    ren = hip_renderer(amd, field, 64)
    ren.occupancy = grid                                           # a grid of the field itself renders
    assert torch.isfinite(ren.render(batch_of(sc))[0]).all()


# ---- training ------------------------------------------------------------------------------------------------------------------------
# Twice the largest fused / eager ratio of final losses in five runs of each side (tools/measure_hashfield_train_k.py, which wrote
# the "training_k" block of profiles/hashfield_parity.json): that ratio is 1.0000141, the run-to-run spread does not show in 40 steps
# on 1024 rays, and so the rule leaves a WEAK bound -- a fused path that trained to twice the eager loss would still pass.  What
# pins the training path to float64 is the gradient parity above; this test says that training moves and lands where eager lands.
TRAIN_K = 2.00003


def training_rays(amd, oracle, synthetic_sd):
    """1024 fixed rays of one teacher view and the teacher's colours."""
    teacher = amd.Network()
    teacher.load_state_dict(synthetic_sd, strict=True)
    teacher = teacher.cuda().eval()
    ids = torch.randperm(400 * 400, generator=torch.Generator().manual_seed(9))[:1024]
    ids = (ids // 400 + 200) * 800 + ids % 400 + 200                # the central 400 x 400 pixels of an 800 x 800 view
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(30.0), pixel_ids=ids)
    o, d = o.float().cuda().contiguous(), d.float().cuda().contiguous()
    with torch.no_grad():
        colors, _ = amd.Renderer(teacher).render({"rays_o": o[None], "rays_d": d[None]})
    return o, d, colors.contiguous()


def training_field(amd, seed=0):
    torch.manual_seed(seed)
    enc = amd.HashEncoder(input_dim=3, num_levels=8, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=14)
    return amd.HashField((-2.0, -2.0, -2.0, 2.0, 2.0, 2.0), encoder=enc).cuda()


def run_fused(amd, rays, steps=40):
    from nerf_replication_amd.training import FusedAdam, train_step
    field = training_field(amd)
    ren = amd.HashRenderer(field)
    ren.N_samples = 64
    opt = FusedAdam(field.parameters(), lr=1e-2)
    return [float(train_step(ren, opt, *rays)) for _ in range(steps)]


def run_eager(amd, rays, steps=40):
    """The same field from the same initial state in eager torch on the same GPU: HashEncoder as it is, nn.Linear layers, torch
    compositing, torch.optim.Adam behind clip_grad_value_(40) (what train_step does for an optimizer that is not FusedAdam)."""
    field = training_field(amd)
    o, d, colors = rays
    t = torch.linspace(2.0, 6.0, 64, device="cuda")
    delta = torch.cat([t[1:] - t[:-1], torch.full((1,), 1e10, device="cuda")])
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    losses = []

    def eager_mlp(net, x):
        for layer in net.layers[:-1]:
            x = torch.relu(layer(x))
        return net.layers[-1](x)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        pts = o[:, None, :] + d[:, None, :] * t[None, :, None]
        geo = eager_mlp(field.sigma_net, field.encoder(pts.reshape(-1, 3), field.wbounds))
        sh = R.sh4(d)
        rgb_raw = eager_mlp(field.color_net, torch.cat([geo, sh[:, None, :].expand(-1, 64, -1).reshape(-1, 16)], dim=1))
        alpha = 1.0 - torch.exp(-torch.relu(geo[:, 0].view(-1, 64)) * delta[None])
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), torch.clamp(1.0 - alpha, 1e-10, 1.0)], dim=1), dim=1)[:, :-1]
        w = T * alpha
        rgb = (w[..., None] * torch.sigmoid(rgb_raw.view(-1, 64, 3))).sum(1) + (1.0 - w.sum(1))[:, None]
        loss = torch.nn.functional.mse_loss(rgb, colors)
        loss.backward()
        torch.nn.utils.clip_grad_value_(field.parameters(), 40.0)
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_training_moves(amd, oracle, synthetic_sd):
    """40 train_step calls with FusedAdam(lr=1e-2) on 1024 fixed teacher rays, L = 8, T = 14, S = 64: the loss falls, and ends at
    most TRAIN_K times where an eager-torch run of the same field from the same initial state ends.  Adam on atomically summed
    gradients diverges from run to run ("Open"), so TRAIN_K is twice the largest ratio (any fused run over any
    eager run) seen in five runs of each side; tools/measure_hashfield_train_k.py makes those runs and writes the ten final losses to
    profiles/hashfield_parity.json under "training_k" (largest ratio 1.0000141: the bound is a weak one, see TRAIN_K)."""
    rays = training_rays(amd, oracle, synthetic_sd)
    fused = run_fused(amd, rays)
    eager = run_eager(amd, rays)
    print(f"fused {fused[0]:.5f} -> {fused[-1]:.5f}   eager {eager[0]:.5f} -> {eager[-1]:.5f}   ratio {fused[-1] / eager[-1]:.3f}")
    R.parity_record("training_moves", {"fused_first": fused[0], "fused_last": fused[-1], "eager_first": eager[0],
                                       "eager_last": eager[-1], "k": TRAIN_K})
    assert abs(fused[0] - eager[0]) <= 1e-4 * eager[0]                # the same field, the same rays
    assert fused[-1] < fused[0]
    assert TRAIN_K is not None and fused[-1] <= TRAIN_K * eager[-1]
