"""-m gpu: the training path (BASELINE config 3), stage by stage against the reference's golden
activations and the CPU oracle under autograd."""
import pytest
import torch

from conftest import parity_record
from gpu_common import amd, rel  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net(amd, synthetic_sd):
    n = amd.Network()
    n.load_state_dict(synthetic_sd, strict=True)
    return n.cuda().eval()


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_forward_save_matches_reference_activations(amd, net, golden, precision):
    """SAVE-mode forward: every tensor autograd would keep for NeRF.forward (network.py:49-74) equals
    the reference's own per-layer activations (forward hooks in oracle/gen_golden.py)."""
    g = golden("mlp_layers.npz")
    L = amd._lib
    P = 128
    net.precision = precision
    prec = L.PRECISIONS[precision]
    o, d = g["pts"].cuda().contiguous(), g["viewdirs"].cuda().contiguous()     # one-sample rays: x = o + d*0
    t = torch.zeros(P, 1, device="cuda")
    for model, tag in (("", "coarse"), ("fine", "fine")):
        raw = torch.empty(P, 1, 4, device="cuda")
        save = torch.full((int(L.call("nerf_train_save_floats", P)),), float("nan"), device="cuda")
        L.call("nerf_mlp_forward_rays_save", o, d, t, 1, P, 1, net.packed(model), raw, save, prec)
        sv = save.cpu()
        rows = P * (96 + 2304 + 128)                   # (P is a multiple of 32: no padding rows)
        assert torch.isfinite(sv[:rows]).all()
        pe, dpe = sv[:P * 64].view(P, 64), sv[P * 64:P * 96].view(P, 32)
        assert (pe[:, :63] - g["emb"][:, :63]).abs().max() <= 5e-7 and torch.all(pe[:, 63] == 0)
        # rays_d / ||rays_d|| in-kernel may differ from the fixture's direction by an ulp, x8 at octave 3
        assert (dpe[:, :27] - g["emb"][:, 63:]).abs().max() <= 2e-6 and torch.all(dpe[:, 27:] == 0)
        for l in range(8):
            h = sv[P * (96 + 256 * l):P * (96 + 256 * (l + 1))].view(P, 256)
            assert rel(h, g[f"{tag}_h{l}"]) <= 2e-5, l
        f = sv[P * (96 + 2048):P * (96 + 2304)].view(P, 256)
        hv = sv[P * (96 + 2304):rows].view(P, 128)
        assert rel(f, g[f"{tag}_feature"]) <= 2e-5 and rel(hv, g[f"{tag}_views"]) <= 2e-5
        assert rel(raw[:, 0], g[f"{tag}_out"]) <= 2e-5
        if precision in ("f32", "f32x"):
            # behind the rows (both SAVE forwards, same layout): ReLU sign bits in accumulator layout, one 1-KiB block per
            # 32-point tile and masked tensor (h0..h7, views)
            bits = sv[rows:rows + (P // 32) * 9 * 256].view(torch.int32).view(P // 32, 9, 64, 4)
            lane = torch.arange(64)
            pt, hh = lane & 31, lane >> 5
            for which, key, ntile in [(l, f"{tag}_h{l}", 8) for l in range(8)] + [(8, f"{tag}_views", 4)]:
                act = g[key].view(P // 32, 32, -1)
                for ti in range(ntile):
                    for r in range(16):
                        feat = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * hh                      # act_feat(t, r, h)
                        want = act[:, pt, feat] > 0                                         # [tiles, 64]
                        got = (bits[:, which, :, ti >> 1] >> (16 * (ti & 1) + r)) & 1
                        # (an activation within rounding of 0 may differ in sign between the GPU and the fixture)
                        near0 = act[:, pt, feat].abs() < 1e-6
                        assert torch.all((got.bool() == want) | near0), (tag, which, ti, r)
    net.precision = "f32"


# Every row of csrc/nerf_wgrad_table.h at its smallest shapes: the five small-layer rows (256 x 64 is what `aligned` lets reach
# the PE -> 256 row), then one shape per generic row that the larger cases below do not reach.  Point counts: a half-empty pair,
# one short of a ring group (32 points), exactly one group, the fallback just past it, two groups
_WGRAD_ROW_SHAPES = [(256, 64), (128, 256), (128, 27), (1, 256), (3, 128),
                     (33, 27), (33, 33), (64, 64), (64, 128), (65, 97), (128, 128)]
_WGRAD_ROW_CASES = [(n_out, n_in, P) for n_out, n_in in _WGRAD_ROW_SHAPES for P in (1, 31, 32, 33, 64)]


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("n_out,n_in,P", [(256, 256, 4099), (256, 63, 777), (128, 256, 1000), (128, 27, 333),
                                           (3, 128, 2050), (1, 256, 513), (256, 256, 1), (256, 256, 200001),
                                           (256, 256, 4096), (256, 256, 200000), (256, 256, 48),     # multiples of 16: asm-load kernel
                                           (256, 256, 16), (256, 256, 17)] + _WGRAD_ROW_CASES)      # one ring group; the <4,4> fallback
def test_wgrad_gemm(amd, n_out, n_in, P, aligned):
    """grad_weight = grad_out^T @ input and grad_bias = grad_out.sum(0), written into a column block of an
    nn.Linear-shaped [out, in_total] gradient (the skip / view concatenations are column blocks)."""
    L = amd._lib
    gen = torch.Generator().manual_seed(n_out * 1000 + n_in)
    # aligned: leading dimensions / offsets that allow the float4 fast path of the 256x256 layers
    ldz, zc0, ldh, hc0, ldw, wc0 = (n_out + 8, 4, n_in + 12, 8, n_in + 11, 7) if aligned else (n_out + 5, 2, n_in + 9, 4, n_in + 11, 7)
    dz = torch.randn(P, ldz, generator=gen)
    hin = torch.randn(P, ldh, generator=gen)
    dw = torch.zeros(n_out, ldw, device="cuda")
    db = torch.zeros(n_out, device="cuda")
    dz_d, hin_d = dz.cuda(), hin.cuda()            # keep the device copies alive across the call
    L.call("nerf_wgrad", dz_d, ldz, zc0, n_out, hin_d, ldh, hc0, n_in, dw, ldw, wc0, db, P)
    ref = dz[:, zc0:zc0 + n_out].double().T @ hin[:, hc0:hc0 + n_in].double()
    got = dw.cpu()
    assert torch.all(got[:, :wc0] == 0) and torch.all(got[:, wc0 + n_in:] == 0)          # only the column block
    scale = ref.abs().max().clamp_min(1e-6)
    assert ((got[:, wc0:wc0 + n_in].double() - ref).abs().max() / scale) <= 2e-5
    assert ((db.cpu().double() - dz[:, zc0:zc0 + n_out].double().sum(0)).abs().max() / scale) <= 2e-5


# (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias: the layouts mlp_backward_impl hands to nerf_wgrad for the small layers
_SMALL_LAYOUTS = {"rgb_linear": ((4, 0, 3), (128, 0, 128), (128, 0), True),
                  "alpha_linear": ((4, 3, 1), (256, 0, 256), (256, 0), True),
                  "views_feature": ((128, 0, 128), (256, 0, 256), (283, 0), True),
                  "views_dirs": ((128, 0, 128), (32, 0, 27), (283, 256), False),
                  "pe_skip": ((256, 0, 256), (64, 0, 63), (319, 0), True),
                  "pe_layer0": ((256, 0, 256), (64, 0, 63), (63, 0), True)}


@pytest.mark.parametrize("P", [64, 192 * 64, 64 * 257, 64 * 1031, 100])       # whole 64-point groups: the asm-ring kernels (1 group; even and
@pytest.mark.parametrize("layer", sorted(_SMALL_LAYOUTS))                      # uneven splits over 256 workgroups); 100: the C++ fallback
def test_wgrad_small_layers_in_training_layout(amd, layer, P):
    """The small-layer weight gradients in exactly the row pitches / column offsets of a training step.  Columns that
    exist in memory but not in the layer (float 63 of a PE row, 27..31 of a direction row, the colour columns next to
    sigma) hold NaN here: they may be loaded but must not reach any output."""
    L = amd._lib
    (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias = _SMALL_LAYOUTS[layer]
    gen = torch.Generator().manual_seed(P + n_out)
    dz = torch.randn(P, ldz, generator=gen)
    hin = torch.randn(P, ldh, generator=gen)
    hin_d = hin.clone()
    hin_d[:, hc0 + n_in:] = float("nan")
    dw = torch.zeros(n_out, ldw, device="cuda")
    db = torch.zeros(n_out, device="cuda")
    dz_d, hin_d = dz.cuda(), hin_d.cuda()
    L.call("nerf_wgrad", dz_d, ldz, zc0, n_out, hin_d, ldh, hc0, n_in, dw, ldw, wc0, db if bias else None, P)
    ref = dz[:, zc0:zc0 + n_out].double().T @ hin[:, hc0:hc0 + n_in].double()
    got = dw.cpu()
    assert torch.all(got[:, :wc0] == 0) and torch.all(got[:, wc0 + n_in:] == 0)
    scale = ref.abs().max().clamp_min(1e-6)
    assert ((got[:, wc0:wc0 + n_in].double() - ref).abs().max() / scale) <= 2e-5
    if bias:
        assert ((db.cpu().double() - dz[:, zc0:zc0 + n_out].double().sum(0)).abs().max() / scale) <= 2e-5
    else:
        assert torch.all(db == 0)


@pytest.mark.parametrize("gscale", [1.0, 1e-7])          # mean-reduced losses hand over gradients around 1e-6 .. 1e-8
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("model,prefix", [("fine", "model_fine"), ("", "model")])
def test_mlp_backward_matches_autograd(amd, net, oracle, synthetic_sd, model, prefix, precision, gscale):
    """loss = sum(raw * G): all 24 parameter gradients of one NeRF MLP and d loss / d t through the
    points (positional encoding included) against the CPU oracle under torch autograd."""
    L = amd._lib
    gen = torch.Generator().manual_seed(7)
    n, S = 37, 5                                              # 185 points: ragged last tile
    o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous()
    d = torch.randn(n, 3, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous()
    t = (torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, dim=-1).values).contiguous()
    G = torch.randn(n, S, 4, generator=gen) * gscale
    G[3] = 0.0                                              # a ray that contributes no gradient
    # ---- oracle
    sd = {k: v.clone().requires_grad_(k.startswith(prefix + ".")) for k, v in synthetic_sd.items()}
    t_ref = t.clone().requires_grad_(True)
    pts = o[:, None, :] + d[:, None, :] * t_ref[:, :, None]
    raw_ref = oracle.network_forward(sd, pts, d / torch.norm(d, dim=-1, keepdim=True), model)
    (raw_ref * G).sum().backward()
    # ---- HIP
    sub = net.model_fine if model == "fine" else net.model
    params = [p.detach().contiguous() for p in sub.ordered_params()]
    prec = L.PRECISIONS[precision]
    pk_b = torch.empty(int(L.call("nerf_packed_bwd_bytes", prec)), dtype=torch.uint8, device="cuda")
    L.call("nerf_pack_model_bwd", params, pk_b, prec)
    P = n * S
    od, dd, td, Gd = o.cuda(), d.cuda(), t.cuda(), G.cuda().contiguous()
    raw = torch.empty(n, S, 4, device="cuda")
    save = torch.empty(int(L.call("nerf_train_save_floats", P)), device="cuda")
    gsave = torch.empty(int(L.call("nerf_train_grad_floats", P)), device="cuda")
    g_t = torch.empty(n, S, device="cuda")
    L.call("nerf_mlp_forward_rays_save", od, dd, td, S, n, S, net.packed(model), raw, save, 0)
    grads = [torch.zeros_like(p) for p in params]
    L.call("nerf_mlp_backward", od, dd, td, S, n, S, pk_b, Gd, save, gsave, g_t, grads, prec)
    torch.cuda.synchronize()
    assert rel(raw, raw_ref.detach()) <= 2e-5
    names = [f"{prefix}.{k}" for k in oracle.SUBMODEL_KEYS]
    worst = 0.0
    for name, got in zip(names, grads):
        ref = sd[name].grad
        err = rel(got, ref)
        worst = max(worst, err)
        assert err <= 1e-5, (name, err)          # measured <= 1.2e-6 (profiles/parity_r03.json)
    e_t = rel(g_t, t_ref.grad)
    print(f"{prefix} [{precision}, |G|~{gscale:g}]: worst parameter-gradient error {worst:.2e}, d/dt error {e_t:.2e}")
    parity_record("gradients", f"mlp_backward_vs_autograd/{prefix}/{precision}/G{gscale:g}",
                  {"worst_param_rel_err": worst, "dt_rel_err": e_t})
    assert e_t <= 1e-5


def test_composite_backward_matches_autograd(amd, oracle, golden):
    g = golden("sampling.npz")
    L = amd._lib
    gen = torch.Generator().manual_seed(11)
    n, S = 200, 192
    raw = g["raw_fine"][:n].clone()
    raw[:, :, 3] = raw[:, :, 3] * 0.2                       # keep rays semi-transparent: gradients everywhere
    t = g["t_sorted"][:n].clone()
    G_rgb, G_dep = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)
    raw_r, t_r = raw.clone().requires_grad_(True), t.clone().requires_grad_(True)
    rgb, dep = oracle.composite(raw_r, t_r, True)
    ((rgb * G_rgb).sum() + (dep * G_dep).sum()).backward()
    rawd, td = raw.cuda().contiguous(), t.cuda().contiguous()
    Gr, Gd = G_rgb.cuda().contiguous(), G_dep.cuda().contiguous()
    g_raw, g_t = torch.empty(n, S, 4, device="cuda"), torch.empty(n, S, device="cuda")
    L.call("nerf_composite_backward", rawd, td, S, n, S, 1, Gr, Gd, g_raw, g_t)
    e_raw, e_t = rel(g_raw, raw_r.grad), rel(g_t, t_r.grad)
    print(f"composite backward: g_raw {e_raw:.2e}, g_t {e_t:.2e}")
    parity_record("gradients", "composite_backward_vs_autograd", {"g_raw_rel_err": e_raw, "g_t_rel_err": e_t})
    assert e_raw <= 1e-5 and e_t <= 1e-5          # measured 1.1e-6 / 2.0e-6


def test_sample_backward_matches_autograd(amd, oracle, golden):
    g = golden("sampling.npz")
    L = amd._lib
    gen = torch.Generator().manual_seed(12)
    n = 256
    raw_c = g["raw_coarse"][:n].clone()
    G = torch.randn(n, 192, generator=gen)
    raw_r = raw_c.clone().requires_grad_(True)
    t_c = oracle.stratified_t().expand(n, 64)
    t_f = oracle.fine_sample(torch.relu(raw_r[..., 3]), t_c)
    t_sorted, _ = torch.sort(torch.cat([t_c, t_f], 1), dim=-1)
    (t_sorted * G).sum().backward()
    rawd = raw_c.cuda().contiguous()
    tcd, ud = torch.linspace(2.0, 6.0, 64).cuda(), torch.linspace(0.0, 1.0, 128).cuda()
    ts = torch.empty(n, 192, device="cuda")
    L.call("nerf_sample_fine", rawd, tcd, ud, n, ts, None, None, 0.0, 0.0)
    Gd = G.cuda().contiguous()
    g_raw = torch.full((n, 64, 4), float("nan"), device="cuda")
    L.call("nerf_sample_fine_backward", rawd, tcd, ud, n, ts, Gd, g_raw)
    got, ref = g_raw.cpu(), raw_r.grad
    assert torch.all(got[..., :3] == 0)
    # per-ray comparison: a searchsorted / denom<1e-5 flip (module docstring of test_gpu_parity) changes a ray's
    # gradient discontinuously, so require 98 % of the rays to agree tightly
    scale = ref[..., 3].abs().amax(dim=1).clamp_min(1e-6)
    err = (got[..., 3] - ref[..., 3]).abs().amax(dim=1) / scale
    print(f"sample backward: median ray error {err.median():.2e}, rays within 1e-3: {(err <= 1e-3).float().mean():.3f}")
    parity_record("gradients", "sample_fine_backward/sampling.npz/256", {
        "median_ray_err": err.median().item(), "q90_ray_err": torch.quantile(err, 0.9).item(), "max_ray_err": err.max().item(),
        "rays_within_1e-3": int((err <= 1e-3).sum()), "rays_within_1e-4": int((err <= 1e-4).sum()), "n_rays": n})
    # measured: 254 of 256 rays within 1e-3, 243 within 1e-4, median 5.6e-6
    assert (err <= 1e-3).float().mean() >= 0.98 and (err <= 1e-4).float().mean() >= 0.90 and err.median() <= 5e-5


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_training_step_matches_reference_autograd(amd, synthetic_sd, golden, precision):
    """The reference's own training semantics: MSE on the fine RGB of a 64-ray batch,
    loss.backward() -- loss and all 48 gradients from oracle/gen_golden.py's autograd fixture."""
    g = golden("autograd.npz")
    net = amd.Network()
    net.load_state_dict(synthetic_sd, strict=True)
    net = net.cuda().train()
    net.precision = precision            # "f32x": forward on split-fp16 MFMA, backward kernels fp32 MFMA
    ren = amd.Renderer(net)
    rgb, dep = ren.render({"rays_o": g["rays_o"][None].cuda(), "rays_d": g["rays_d"][None].cuda()})
    assert rgb.requires_grad
    loss = torch.nn.functional.mse_loss(rgb, g["gt"].cuda())
    loss.backward()
    assert abs(loss.item() - g["loss"].item()) <= 1e-6 * max(1.0, abs(g["loss"].item()))
    assert (rgb.detach().cpu() - g["rgb"]).abs().max() <= 2e-3
    rows = []
    for k, p in net.named_parameters():
        ref = g["grad/" + k]
        assert p.grad is not None and p.grad.shape == ref.shape, k
        denom = ref.abs().max().item()
        err = (p.grad.cpu() - ref).abs().max().item()
        rows.append((k, err / denom if denom > 0 else err, denom))
    worst = max(rows, key=lambda r: r[1])
    fine = max(r[1] for r in rows if r[0].startswith("model_fine."))
    coarse = max(r[1] for r in rows if r[0].startswith("model."))
    print(f"training step: loss {loss.item():.6f}; worst relative gradient error fine {fine:.2e}, coarse {coarse:.2e} ({worst[0]})")
    parity_record("gradients", f"training_step_vs_reference_autograd/64rays/{precision}", {
        "loss": loss.item(), "loss_ref": g["loss"].item(), "rgb_max_err": (rgb.detach().cpu() - g["rgb"]).abs().max().item(),
        "fine_worst_rel_err": fine, "coarse_worst_rel_err": coarse, "worst_tensor": worst[0],
        "per_tensor_rel_err": {k: e for k, e, _ in rows}})
    # the fine model's gradients are smooth in the rounding; the coarse model's go through the inverse-CDF
    # sampler, whose index / `denom < 1e-5` flips make single rays jump (the reference's own discontinuity)
    # measured (profiles/parity_r03.json): fine 1.2e-4 (f32) / 1.6e-4 (f32x), coarse 5.1e-3 / 8.6e-3 -> ~3x
    assert fine <= 5e-4 and coarse <= 2.5e-2
    # coarse colour layers receive exactly zero gradient: the coarse RGB is never composited
    for k in ("model.rgb_linear.weight", "model.views_linears.0.weight", "model.feature_linear.weight"):
        assert torch.all(dict(net.named_parameters())[k].grad == 0), k


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_short_training_run_reduces_loss(amd, oracle, synthetic_sd, precision):
    """Config-3-shaped loop (render -> MSE on fine RGB -> backward -> clip 40 -> Adam): the fine colour
    head is knocked off a target image and trained back; the loss must fall, which also exercises the
    re-packing of the weight streams after every optimizer step."""
    from nerf_replication_amd.training import train_step
    torch.manual_seed(0)
    net = amd.Network()
    net.load_state_dict(synthetic_sd, strict=True)
    net = net.cuda().train()
    net.precision = precision
    ren = amd.Renderer(net)
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(9))[:1024]
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(20.0), pixel_ids=ids)
    o, d = o.cuda(), d.cuda()
    with torch.no_grad():
        net.eval()
        target, _ = ren.render({"rays_o": o[None], "rays_d": d[None]})
        net.train()
        for p in net.model_fine.rgb_linear.parameters():
            p.add_(0.5 * torch.randn_like(p))
    head = list(net.model_fine.rgb_linear.parameters())
    opt = torch.optim.Adam(head, lr=2e-2, eps=1e-8)
    before = [p.detach().clone() for p in net.model_fine.pts_linears[3].parameters()]
    losses = [train_step(ren, opt, o, d, target).item() for _ in range(25)]
    print(f"losses [{precision}]", ["%.5f" % l for l in losses[::4]])
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < 0.25 * losses[0]
    for b, p in zip(before, net.model_fine.pts_linears[3].parameters()):
        assert torch.equal(b, p.detach()) and p.grad is not None          # not in the optimizer: untouched, but has a gradient


def test_fused_adam_matches_torch_adam(amd):
    """nerf_adam_step (clip 40 + Adam) against clip_grad_value_ + torch.optim.Adam, the reference's stock
    optimizer (optimizer.py:21-24, trainer.py:59), over several steps with a changing learning rate."""
    from nerf_replication_amd.training import FusedAdam
    gen = torch.Generator().manual_seed(3)
    shapes = [(256, 63), (256,), (128, 283), (3, 128), (1,)]
    ref = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone().cuda()) for p in ref]
    opt_ref = torch.optim.Adam(ref, lr=5e-4, eps=1e-8, weight_decay=0.0)
    opt = FusedAdam(mine, lr=5e-4, eps=1e-8, weight_decay=0.0, clip_value=40.0)
    for step in range(6):
        lr = FusedAdam.exponential_lr(5e-4, epoch=step * 40)
        for g in opt_ref.param_groups:
            g["lr"] = lr
        opt.lr = lr
        for p, q in zip(ref, mine):
            gr = torch.randn(p.shape, generator=gen) * (100.0 if step % 2 else 0.01)      # some steps need the clip
            p.grad = gr.clone()
            q.grad = gr.cuda()
        torch.nn.utils.clip_grad_value_(ref, 40.0)
        opt_ref.step()
        v0 = mine[0]._version
        opt.step()
        assert mine[0]._version > v0
    for p, q in zip(ref, mine):
        assert (q.detach().cpu() - p.detach()).abs().max() <= 2e-6 * max(1.0, p.detach().abs().max().item())
    assert abs(FusedAdam.exponential_lr(5e-4, 500) - 5e-5) < 1e-12


@pytest.mark.gpu
def test_checkpoint_resume_continues_bit_identically(amd, tmp_path):
    """save_model / load_model (reference layout, net_utils.py:288-343) round-trip the network AND the fused
    optimizer: two steps, save, reload into fresh objects, one more step == three uninterrupted steps."""
    from nerf_replication_amd.training import FusedAdam
    gen = torch.Generator().manual_seed(5)

    def grads_for(step, params):
        g = torch.Generator().manual_seed(100 + step)
        return [torch.randn(p.shape, generator=g).cuda() * 0.05 for p in params]

    def fresh():
        net = amd.Network()
        torch.manual_seed(0)
        for p in net.parameters():
            p.data = torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.1
        return net.cuda()

    net_a = fresh(); opt_a = FusedAdam(net_a.parameters(), lr=5e-4)
    for step in range(3):
        for p, g in zip(net_a.parameters(), grads_for(step, list(net_a.parameters()))):
            p.grad = g
        opt_a.step()

    net_b = fresh(); opt_b = FusedAdam(net_b.parameters(), lr=5e-4)
    for step in range(2):
        for p, g in zip(net_b.parameters(), grads_for(step, list(net_b.parameters()))):
            p.grad = g
        opt_b.step()
    amd.save_model(net_b, opt_b, None, None, str(tmp_path), epoch=1, last=True)
    net_c = amd.Network().cuda(); opt_c = FusedAdam(net_c.parameters(), lr=1.0)
    assert amd.load_model(net_c, opt_c, None, None, str(tmp_path)) == 2
    assert opt_c.step_count == 2 and opt_c.lr == 5e-4
    for p, g in zip(net_c.parameters(), grads_for(2, list(net_c.parameters()))):
        p.grad = g
    opt_c.step()
    for pa, pc in zip(net_a.parameters(), net_c.parameters()):
        assert torch.equal(pa.detach(), pc.detach())


@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("model,prefix", [("fine", "model_fine"), ("", "model")])
def test_network_forward_is_differentiable(amd, oracle, synthetic_sd, model, prefix, precision):
    """Network.forward itself under autograd (reference: network.py:199-258 is an ordinary differentiable module):
    loss = sum(raw * G) -> gradients of the 24 tensors of the selected sub-model AND of `inputs` and `viewdirs`, against
    oracle.network_forward under torch autograd.  viewdirs are deliberately NOT unit length: Network.forward uses them
    as given (only the renderer normalises, volume_renderer.py:314).  Also the masked (ESS/ERT) call."""
    gen = torch.Generator().manual_seed(17)
    n, S = 9, 7                                               # 63 points: ragged tile
    pts = (torch.rand(n, S, 3, generator=gen) * 2 - 1) * 2.5
    vd = torch.randn(n, 3, generator=gen) * 0.7
    G = torch.randn(n, S, 4, generator=gen)
    mask = torch.rand(n, S, generator=gen) > 0.35
    net = amd.Network()
    net.load_state_dict(synthetic_sd, strict=True)
    net = net.cuda().train()
    net.precision = precision
    sub = net.model_fine if model == "fine" else net.model
    other = net.model if model == "fine" else net.model_fine
    names = [f"{prefix}.{k}" for k in oracle.SUBMODEL_KEYS]
    for tag, msk in (("unmasked", None), ("masked", mask)):
        # ---- oracle
        sd = {k: v.clone().requires_grad_(k.startswith(prefix + ".")) for k, v in synthetic_sd.items()}
        p_ref = pts.clone().requires_grad_(True)
        vd_ref = vd.clone().requires_grad_(True)
        raw_ref = oracle.network_forward(sd, p_ref, vd_ref, model)
        if msk is not None:
            raw_ref = raw_ref * msk[..., None]                # network.py:238-253: zeros where masked out
        (raw_ref * G).sum().backward()
        # ---- HIP through nn.Module.__call__
        net.zero_grad(set_to_none=True)
        p_hip = pts.cuda().requires_grad_(True)
        vd_hip = vd.cuda().requires_grad_(True)
        raw = net(p_hip, vd_hip, None if msk is None else msk.cuda(), model)
        assert raw.requires_grad and raw.shape == (n, S, 4)
        (raw * G.cuda()).sum().backward()
        assert rel(raw.detach(), raw_ref.detach()) <= 2e-5
        worst = 0.0
        for name, p in zip(names, sub.ordered_params()):
            err = rel(p.grad, sd[name].grad)
            worst = max(worst, err)
            assert err <= 1e-5, (tag, name, err)         # measured <= 1.3e-6
        e_x = rel(p_hip.grad, p_ref.grad)
        assert e_x <= 1e-5, (tag, e_x)
        e_d = rel(vd_hip.grad, vd_ref.grad)                                  # d / d viewdirs (nerf_viewdirs_backward)
        assert vd_hip.grad.shape == (n, 3) and e_d <= 1e-5, (tag, e_d)
        assert all(p.grad is None for p in other.parameters())               # the other sub-model is not touched
        if msk is not None:
            assert torch.all(p_hip.grad.cpu()[~msk] == 0) and torch.all(raw.detach().cpu()[~msk] == 0)
        parity_record("gradients", f"network_forward_autograd/{prefix}/{precision}/{tag}",
                      {"worst_param_rel_err": worst, "d_inputs_rel_err": e_x, "d_viewdirs_rel_err": e_d})
    # eval() + no_grad stays the inference kernel; grad w.r.t. inputs alone works on an eval() network too
    net.eval()
    with torch.no_grad():
        assert not net(pts.cuda(), vd.cuda(), None, model).requires_grad
    p_hip = pts.cuda().requires_grad_(True)
    net(p_hip, vd.cuda(), None, model).sum().backward()
    assert p_hip.grad is not None and torch.isfinite(p_hip.grad).all()


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_density_only_pair_equals_full_pair_with_zero_colour_gradient(amd, net, synthetic_sd, precision):
    """The coarse pass of a training step runs nerf_mlp_forward_rays_save_density / nerf_mlp_backward_density (the colour
    branch is computed by the reference but never used: SURVEY F6/F10).  Against the full pair fed a d loss / d raw with
    zero rgb columns: sigma bit-identical, the 18 trunk / alpha gradients and d loss / d t equal to rounding (the
    weight-gradient kernels accumulate with atomics), the colour-branch gradients EXACTLY zero in both."""
    L = amd._lib
    gen = torch.Generator().manual_seed(23)
    n, S = 41, 64
    o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous().cuda()
    d = torch.randn(n, 3, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous().cuda()
    t_c = torch.linspace(2.0, 6.0, S).cuda()
    G = torch.randn(n, S, 4, generator=gen) * 1e-3
    G[..., :3] = 0.0
    G = G.cuda().contiguous()
    params = [p.detach().contiguous() for p in net.model.ordered_params()]
    prec = L.PRECISIONS[precision]                           # (f32x: both instances since round 3)
    net.precision = precision
    pk_b = torch.empty(int(L.call("nerf_packed_bwd_bytes", prec)), dtype=torch.uint8, device="cuda")
    L.call("nerf_pack_model_bwd", params, pk_b, prec)
    P = n * S
    out = {}
    for tag, fwd, bwd in (("full", "nerf_mlp_forward_rays_save", "nerf_mlp_backward"),
                          ("density", "nerf_mlp_forward_rays_save_density", "nerf_mlp_backward_density")):
        raw = torch.full((n, S, 4), float("nan"), device="cuda")
        save = torch.empty(int(L.call("nerf_train_save_floats", P)), device="cuda")
        gsave = torch.empty(int(L.call("nerf_train_grad_floats", P)), device="cuda")
        g_t = torch.empty(n, S, device="cuda")
        grads = [torch.zeros_like(p) for p in params]
        L.call(fwd, o, d, t_c, 0, n, S, net.packed(""), raw, save, prec)
        L.call(bwd, o, d, t_c, 0, n, S, pk_b, G, save, gsave, g_t, grads, prec)
        torch.cuda.synchronize()
        out[tag] = (raw, g_t, grads)
    assert torch.equal(out["full"][0][..., 3], out["density"][0][..., 3])
    assert torch.all(out["density"][0][..., :3] == 0)
    assert rel(out["density"][1], out["full"][1].cpu()) <= 1e-6
    names = list(__import__("nerf_oracle").SUBMODEL_KEYS)
    for name, gf, gd in zip(names, out["full"][2], out["density"][2]):
        if name.startswith(("views_linears", "feature_linear", "rgb_linear")):
            assert torch.all(gf == 0) and torch.all(gd == 0), name
        else:
            assert gf.abs().max() > 0 and rel(gd, gf.cpu()) <= 2e-6, name
    net.precision = "f32"


# 288 tiles; a single tile; 35 tiles (fewer than scan threads); 1026 tiles (more than scan threads: two per thread, 513 threads busy)
@pytest.mark.parametrize("shape", [(48, 192), (1, 32), (7, 160), (171, 192)])
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("density_only", [False, True])
@pytest.mark.parametrize("dead_frac", [0.0, 0.6, 1.0])
def test_dead_tile_skip_changes_nothing(amd, net, synthetic_sd, monkeypatch, dead_frac, density_only, precision, shape):
    """Tiles (32 consecutive points) whose d loss / d raw is zero throughout are dropped from the chain launch and from every
    weight-gradient launch (nerf_tile_flags_kernel -> live-tile list).  Against the same call with NERF_DEAD_TILE_SKIP=0:
    d loss / d t equal as numbers everywhere (bit-identical code on live tiles, 0 on dead ones), all 24 parameter gradients
    equal to the rounding of their atomic accumulation -- for no dead tile, a scene-like 60 %, and all of them (gradients
    exactly zero).  Zeros include -0.0; a tile with ONE live point is live."""
    L = amd._lib
    net.precision = precision
    prec = L.PRECISIONS[precision]
    gen = torch.Generator().manual_seed(31)
    n, S = shape                                              # (48, 192): 288 tiles; with dead_frac 0.6 about 115 stay live
    model = ""
    o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous().cuda()
    d = torch.randn(n, 3, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous().cuda()
    t = torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, dim=-1).values.cuda().contiguous()
    G = torch.randn(n, S, 4, generator=gen) * 1e-3
    tiles = G.view(-1, 32, 4)
    dead = torch.rand(tiles.shape[0], generator=gen) < dead_frac
    tiles[dead] = 0.0
    if dead_frac == 0.6 and int(dead.sum()) >= 2:
        k = int(dead.nonzero()[0])
        tiles[k, 7, 3] = 2e-4                                  # one live point (sigma channel): the tile must run
        tiles[int(dead.nonzero()[1])] = -0.0                   # negative zeros are zeros
    if density_only:
        tiles[..., :3] = 0.0
    G = G.cuda().contiguous()
    params = [p.detach().contiguous() for p in net.model.ordered_params()]
    pk_b = torch.empty(int(L.call("nerf_packed_bwd_bytes", prec)), dtype=torch.uint8, device="cuda")
    L.call("nerf_pack_model_bwd", params, pk_b, prec)
    P = n * S
    fwd = "nerf_mlp_forward_rays_save_density" if density_only else "nerf_mlp_forward_rays_save"
    bwd = "nerf_mlp_backward_density" if density_only else "nerf_mlp_backward"
    raw = torch.empty((n, S, 4), device="cuda")
    save = torch.empty(int(L.call("nerf_train_save_floats", P)), device="cuda")
    L.call(fwd, o, d, t, S, n, S, net.packed(model), raw, save, prec)
    out = {}
    for tag, env in (("skip", "1"), ("dense", "0")):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        gsave = torch.full((int(L.call("nerf_train_grad_floats", P)),), float("nan"), device="cuda")     # dead rows stay NaN: never read
        g_t = torch.full((n, S), float("nan"), device="cuda")
        grads = [torch.zeros_like(p) for p in params]
        L.call(bwd, o, d, t, S, n, S, pk_b, G, save, gsave, g_t, grads, prec)
        torch.cuda.synchronize()
        out[tag] = (g_t, grads)
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")
    net.precision = "f32"
    assert torch.isfinite(out["skip"][0]).all()
    assert torch.all(out["skip"][0] == out["dense"][0])                     # equal as numbers (0 == -0)
    names = list(__import__("nerf_oracle").SUBMODEL_KEYS)
    for name, gs, gd in zip(names, out["skip"][1], out["dense"][1]):
        assert torch.isfinite(gs).all(), name
        if dead_frac == 1.0 or bool(dead.all()):
            assert torch.all(gs == 0) and torch.all(gd == 0), name
        elif density_only and name.startswith(("views_linears", "feature_linear", "rgb_linear")):
            assert torch.all(gs == 0) and torch.all(gd == 0), name
        else:
            assert gd.abs().max() > 0 and rel(gs, gd.cpu()) <= 1e-5, name      # (sums of ~10^4 signed terms, accumulated by atomics in a different order)


@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("family", ["base", "sharp", "trained"])
def test_training_step_same_with_and_without_dead_tile_skipping(amd, family_sd, family, monkeypatch, precision):
    """A whole step (render_with_grad -> MSE -> backward) on scenes with 17 % ... 86 % density-free fine tiles, the product path
    (fine forward stores nothing past h6 for tiles without density, backward on live tiles only) against
    NERF_DEAD_TILE_SKIP=0 (every row stored, every tile computed): rgb / depth bit-identical, all 48 gradients equal to the
    rounding of their atomic accumulation."""
    from nerf_replication_amd.training import render_with_grad
    out = {}
    for tag, env in (("skip", "1"), ("dense", "0")):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        net = amd.Network(); net.load_state_dict(family_sd(family)); net = net.cuda().train(); net.precision = precision
        ren = amd.Renderer(net)
        ren.live_tile_stats = []
        gen = torch.Generator().manual_seed(5)
        n = 160
        d = torch.randn(n, 3, generator=gen) * 0.25 + torch.tensor([0.0, 0.0, -1.0])
        d = (d / d.norm(dim=-1, keepdim=True)).cuda().contiguous()
        o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous().cuda()
        target = torch.rand(n, 3, generator=gen).cuda()
        rgb, dep = render_with_grad(ren, o, d)
        loss = torch.nn.functional.mse_loss(rgb, target)
        loss.backward()
        torch.cuda.synchronize()
        st = ren.live_tile_stats[0]
        out[tag] = (rgb.detach().clone(), dep.detach().clone(), [p.grad.clone() for p in net.parameters()], int(st[0].item()), st[1])
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")
    assert torch.equal(out["skip"][0], out["dense"][0]) and torch.equal(out["skip"][1], out["dense"][1])
    assert out["dense"][3] == -1 and 0 <= out["skip"][3] <= out["skip"][4]
    if family in ("sharp", "trained"):
        assert out["skip"][3] < 0.6 * out["skip"][4]                # these scenes are mostly empty: most fine tiles are dropped
    for gs, gd in zip(out["skip"][2], out["dense"][2]):
        assert torch.isfinite(gs).all()
        if gd.abs().max() == 0:
            assert torch.all(gs == 0)
        else:
            assert rel(gs, gd.cpu()) <= 1e-4            # (atomic accumulation order; scalar sums with cancellation reach 5e-5)


@pytest.mark.parametrize("n_sub", [1, 5, 63])
def test_per_ray_adjoints_are_independent_of_the_ray_count(amd, golden, n_sub):
    """The compositing and sampler adjoints run one wave per ray, four rays per workgroup: a ray count that leaves waves of the
    last workgroup without a ray (1, 5, 63) must give exactly the rows the same rays get inside a larger call; S = 64 and 192
    for compositing (one and three 64-lane chunks; shared and per-ray depth tables)."""
    g = golden("sampling.npz")
    lib, L = amd._lib.load(), amd._lib
    gen = torch.Generator().manual_seed(77)
    st = L.stream_of(torch.device("cuda:0"))
    n_all = 64
    for S, raw_key, t_all, stride in ((192, "raw_fine", g["t_sorted"][:n_all].cuda().contiguous(), 192),
                                      (64, "raw_coarse", torch.linspace(2.0, 6.0, 64).cuda(), 0)):
        raw = g[raw_key][:n_all].clone()
        raw[..., 3] *= 0.2
        raw = raw.cuda().contiguous()
        Gr = torch.randn(n_all, 3, generator=gen).cuda().contiguous()
        Gd = torch.randn(n_all, generator=gen).cuda().contiguous()
        outs = []
        for n in (n_all, n_sub):
            g_raw = torch.full((n_all, S, 4), float("nan"), device="cuda")
            g_t = torch.full((n_all, S), float("nan"), device="cuda")
            L.call("nerf_composite_backward", raw, t_all, stride, n, S, 1, Gr, Gd, g_raw, g_t)
            torch.cuda.synchronize()
            outs.append((g_raw, g_t))
        assert torch.equal(outs[0][0][:n_sub], outs[1][0][:n_sub]) and torch.equal(outs[0][1][:n_sub], outs[1][1][:n_sub])
        assert torch.isnan(outs[1][0][n_sub:]).all() and torch.isnan(outs[1][1][n_sub:]).all()          # nothing written past the count
        assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    raw_c = g["raw_coarse"][:n_all].cuda().contiguous()
    tcd, ud = torch.linspace(2.0, 6.0, 64).cuda(), torch.linspace(0.0, 1.0, 128).cuda()
    ts = torch.empty(n_all, 192, device="cuda")
    L.call("nerf_sample_fine", raw_c, tcd, ud, n_all, ts, None, None, 0.0, 0.0)
    G = torch.randn(n_all, 192, generator=gen).cuda().contiguous()
    outs = []
    for n in (n_all, n_sub):
        g_raw = torch.full((n_all, 64, 4), float("nan"), device="cuda")
        L.call("nerf_sample_fine_backward", raw_c, tcd, ud, n, ts, G, g_raw)
        torch.cuda.synchronize()
        outs.append(g_raw)
    # (LDS float atomics accumulate the few contributions per cdf entry in arbitrary order: equal to rounding, not bit for bit)
    ref, got = outs[0][:n_sub, :, 3], outs[1][:n_sub, :, 3]
    assert ((ref - got).abs().amax(dim=1) <= 1e-5 * ref.abs().amax(dim=1).clamp_min(1e-20)).all()
    assert torch.isnan(outs[1][n_sub:]).all()
    # S > 192 is refused, not silently mis-indexed
    rc = lib.nerf_composite_backward(L.ptr(raw_c), L.ptr(tcd), 0, 1, 193, 1, L.ptr(Gr), None, L.ptr(outs[0]), None, st)
    assert rc != 0 and b"192" in lib.nerf_last_error()


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_network_forward_viewdirs_gradient_with_dead_tiles(amd, oracle, synthetic_sd, precision):
    """Round-2 ADVICE (medium): with n*s a multiple of 32 the point-mode backward runs on the live-tile list and leaves the g_zv
    rows of dead tiles unwritten, while nerf_viewdirs_backward sums g_zv over ALL samples of a ray.  Whole 32-point tiles of the
    incoming gradient are zero here (the normal case under compositing) and `viewdirs.requires_grad`: d/d viewdirs, d/d inputs and
    the 24 parameter gradients against the oracle under autograd; on an eval() network too (the gate honours viewdirs)."""
    gen = torch.Generator().manual_seed(41)
    n, S = 6, 64                                              # 384 points = 12 tiles, two per ray
    pts = (torch.rand(n, S, 3, generator=gen) * 2 - 1) * 2.5
    vd = torch.randn(n, 3, generator=gen) * 0.7
    G = torch.randn(n, S, 4, generator=gen)
    tiles = G.view(-1, 32, 4)
    tiles[[0, 3, 4, 7, 10]] = 0.0                             # ray 0: first half dead; ray 1: second; ray 2: first; ray 3: second; ray 5: first
    tiles[11] = 0.0
    tiles[10] = 0.0                                           # ray 5: BOTH tiles dead -> d/d viewdirs of ray 5 is exactly zero
    net = amd.Network()
    net.load_state_dict(synthetic_sd, strict=True)
    net = net.cuda().train()
    net.precision = precision
    sd = {k: v.clone().requires_grad_(k.startswith("model_fine.")) for k, v in synthetic_sd.items()}
    p_ref, vd_ref = pts.clone().requires_grad_(True), vd.clone().requires_grad_(True)
    (oracle.network_forward(sd, p_ref, vd_ref, "fine") * G).sum().backward()
    for mode in ("train", "eval"):
        net.train(mode == "train")
        net.zero_grad(set_to_none=True)
        # poison the allocator's free blocks: an uninitialised gsave would show up as NaN / 1e30 in the sums
        junk = torch.full((n * S * 2432 + 4096,), float("nan"), device="cuda"); del junk
        p_hip = pts.cuda().requires_grad_(mode == "train")
        vd_hip = vd.cuda().requires_grad_(True)
        raw = net(p_hip, vd_hip, None, "fine")
        assert raw.requires_grad                              # eval(): viewdirs alone switches the autograd path on
        (raw * G.cuda()).sum().backward()
        assert torch.isfinite(vd_hip.grad).all()
        e_d = rel(vd_hip.grad, vd_ref.grad)
        assert e_d <= 1e-5, (mode, e_d)
        assert torch.all(vd_hip.grad[5] == 0) and vd_ref.grad[5].abs().max() == 0
        if mode == "train":
            assert rel(p_hip.grad, p_ref.grad) <= 1e-5
            assert torch.all(p_hip.grad.view(-1, 32, 3)[[0, 3, 4, 7, 10, 11]] == 0)
            for name, p in zip([f"model_fine.{k}" for k in oracle.SUBMODEL_KEYS], net.model_fine.ordered_params()):
                assert rel(p.grad, sd[name].grad) <= 1e-5, name
    parity_record("gradients", f"network_forward_viewdirs_dead_tiles/{precision}", {"d_viewdirs_rel_err": e_d})


def test_network_forward_detects_parameter_update_between_forward_and_backward(amd, synthetic_sd):
    """The parameters are saved through save_for_backward: an in-place update between forward and backward raises autograd's
    version error instead of repacking new weights against activations of the old ones (round-2 ADVICE)."""
    net = amd.Network()
    net.load_state_dict(synthetic_sd, strict=True)
    net = net.cuda().train()
    pts = torch.rand(2, 32, 3, device="cuda")
    vd = torch.rand(2, 3, device="cuda")
    raw = net(pts, vd, None, "")
    with torch.no_grad():
        net.model.alpha_linear.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        raw.sum().backward()


@pytest.mark.parametrize("shape", [(48, 192), (1, 32)])
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("dead_frac", [0.6, 1.0])
def test_point_mode_backward_in_list_mode(amd, net, monkeypatch, dead_frac, precision, shape):
    """nerf_mlp_forward_points_save / nerf_mlp_backward_points on the live-tile list (round-2 ADVICE: untested paths -- the g_x
    memset with dead tiles, nerf_mlp_bwd_f32x_kernel<true> taking four list entries per workgroup, nerf_mlp_bwd_f32_kernel<true>
    with live_tiles) against NERF_DEAD_TILE_SKIP=0: g_pts equal as numbers, the 24 gradients to the rounding of their atomics,
    and the g_zv region (what nerf_viewdirs_backward reads) zero on dead tiles."""
    L = amd._lib
    prec = L.PRECISIONS[precision]
    net.precision = precision
    gen = torch.Generator().manual_seed(53)
    n, S = shape
    P = n * S
    pts = ((torch.rand(n, S, 3, generator=gen) * 2 - 1) * 2.5).cuda().contiguous()
    vd = torch.randn(n, 3, generator=gen)
    vd = (vd / vd.norm(dim=-1, keepdim=True)).cuda().contiguous()
    G = torch.randn(n, S, 4, generator=gen) * 1e-3
    tiles = G.view(-1, 32, 4)
    dead = torch.rand(tiles.shape[0], generator=gen) < dead_frac
    tiles[dead] = 0.0
    G = G.cuda().contiguous()
    params = [p.detach().contiguous() for p in net.model_fine.ordered_params()]
    pk_b = torch.empty(int(L.call("nerf_packed_bwd_bytes", prec)), dtype=torch.uint8, device="cuda")
    L.call("nerf_pack_model_bwd", params, pk_b, prec)
    raw = torch.empty((n, S, 4), device="cuda")
    save = torch.empty(int(L.call("nerf_train_save_floats", P)), device="cuda")
    L.call("nerf_mlp_forward_points_save", pts, vd, n, S, net.packed("fine"), raw, save, prec)
    out = {}
    for tag, env in (("skip", "1"), ("dense", "0")):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        gsave = torch.full((int(L.call("nerf_train_grad_floats", P)),), float("nan"), device="cuda")
        g_x = torch.full((n, S, 3), float("nan"), device="cuda")
        grads = [torch.zeros_like(p) for p in params]
        L.call("nerf_mlp_backward_points", pts, n, S, pk_b, G, save, gsave, g_x, grads, prec)
        torch.cuda.synchronize()
        out[tag] = (g_x, grads, gsave[:P * 128].view(-1, 32, 128).clone())
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")
    net.precision = "f32"
    assert torch.isfinite(out["skip"][0]).all() and torch.all(out["skip"][0] == out["dense"][0])
    assert torch.all(out["skip"][2][dead.cuda()] == 0) and torch.isfinite(out["skip"][2]).all()
    for gs, gd in zip(out["skip"][1], out["dense"][1]):
        assert torch.isfinite(gs).all()
        if bool(dead.all()):
            assert torch.all(gs == 0) and torch.all(gd == 0)
        else:
            assert gd.abs().max() > 0 and rel(gs, gd.cpu()) <= 1e-5


def test_dense_backward_refuses_a_forward_that_skipped_rows(amd, net, family_sd, monkeypatch):
    """One helper decides about dead-tile skipping for the SAVE forward and for the backward pass, and the forward stamps the save
    buffer.  If the two are forced apart anyway (environment toggled between the passes), the dense backward does not read the
    rows that were never written in silence: grads[alpha_linear.bias] comes back NaN."""
    L = amd._lib
    n, S = 32, 192
    P = n * S
    sharp = amd.Network(); sharp.load_state_dict(family_sd("sharp")); sharp = sharp.cuda().eval()
    gen = torch.Generator().manual_seed(3)
    o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous().cuda()
    d = torch.randn(n, 3, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous().cuda()
    t = torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, dim=-1).values.cuda().contiguous()
    params = [p.detach().contiguous() for p in sharp.model_fine.ordered_params()]
    pk_b = torch.empty(int(L.call("nerf_packed_bwd_bytes", 0)), dtype=torch.uint8, device="cuda")
    L.call("nerf_pack_model_bwd", params, pk_b, 0)
    raw = torch.empty((n, S, 4), device="cuda")
    save = torch.zeros(int(L.call("nerf_train_save_floats", P)), device="cuda")
    monkeypatch.setenv("NERF_DEAD_TILE_SKIP", "1")
    L.call("nerf_mlp_forward_rays_save_for_compositing", o, d, t, S, n, S, sharp.packed("fine"), raw, save, 0)
    G = torch.zeros(n, S, 4, device="cuda")
    G[..., 3] = (raw[..., 3] > 0).float() * 1e-3               # the contract: zero wherever sigma <= 0
    res = {}
    for env in ("1", "0"):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        gsave = torch.zeros(int(L.call("nerf_train_grad_floats", P)), device="cuda")
        g_t = torch.zeros(n, S, device="cuda")
        grads = [torch.zeros_like(p) for p in params]
        L.call("nerf_mlp_backward", o, d, t, S, n, S, pk_b, G, save, gsave, g_t, grads, 0)
        torch.cuda.synchronize()
        res[env] = grads[21]                                  # alpha_linear.bias
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")
    assert torch.isfinite(res["1"]).all()
    assert torch.isnan(res["0"]).all()
