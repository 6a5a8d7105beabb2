"""-m gpu: training with fast_sampling (the ESS / ERT masked fine pass on compacted points) and with N_importance = 0
(coarse only), against the reference's own autograd (tests/golden/masked_train.npz, tools/gen_masked_train_golden.py) and
against the unmasked entries of the C ABI."""
import pytest
import torch

from conftest import parity_record
from gpu_common import amd, assert_grads_equal, network  # noqa: F401
from train_steps_common import subsample

pytestmark = pytest.mark.gpu

MASKED_CASES = (("trained_t002", "trained", 0.02), ("sharp_t025", "sharp", 0.25), ("trained_t025", "trained", 0.25))
GRAD_STRIDE = 53


def _case(golden, tag):
    g = golden("masked_train.npz")
    assert int(g["grad_stride"]) == GRAD_STRIDE
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + "/")}


def _grad_rows(net, c, prefixes=("model.", "model_fine.")):
    rows = []
    for k, p in net.named_parameters():
        if not k.startswith(prefixes):
            continue
        ref = c["grad/" + k]
        assert p.grad is not None, k
        got = subsample(p.grad.cpu(), GRAD_STRIDE)
        assert got.shape == ref.shape, k
        denom = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        rows.append((k, err / denom if denom > 0 else err, denom))
    return rows


# ================================================================================ 1 + 4: step parity with the reference, points evaluated
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("tag,family,thr", MASKED_CASES)
def test_masked_step_matches_reference_autograd(amd, family_sd, golden, tag, family, thr, precision):
    """The reference's step with fast_sampling (MSE on the fine RGB of 96 rays, loss.backward()): the mask, the loss, rgb and
    the 48 gradients of the fixture.  The fixture keeps only rays whose reference mask is stable under perturbations of the
    coarse sigma ten times the recorded GPU-vs-reference deviation (tools/gen_masked_train_golden.py), so the mask must be
    EQUAL, on every ray.  Bounds: those of test_training_step_matches_reference_autograd (the same kernels on a subset of
    the points): loss 1e-6 relative, rgb 2e-3, worst relative gradient error per tensor fine 5e-4 / coarse 2.5e-2 (the coarse
    gradients go through the inverse-CDF sampler's own discontinuities).  masked_stats reports M = 64 n + valid_fine.sum()."""
    c = _case(golden, tag)
    assert float(c["weights_threshold"]) == pytest.approx(thr)
    net = network(amd, family_sd(family), precision, train=True)
    ren = amd.Renderer(net)
    ren.fast_sampling, ren.weights_threshold = True, thr
    ren.masked_stats, ren.capture_adjoints = [], {}
    rgb, dep = ren.render({"rays_o": c["rays_o"][None].cuda(), "rays_d": c["rays_d"][None].cuda()})
    assert rgb.requires_grad
    loss = torch.nn.functional.mse_loss(rgb, c["target"].cuda())
    loss.backward()
    torch.cuda.synchronize()
    valid = ren.capture_adjoints["valid_sorted"].cpu()
    n_flipped = int((valid != c["valid_sorted"]).sum())
    sig = ren.capture_adjoints["raw_coarse"][..., 3].cpu()
    sig_err = (sig - c["sigma_coarse_raw"]).abs().max().item() / (c["sigma_coarse_raw"].max() - c["sigma_coarse_raw"].min()).item()
    rows = _grad_rows(net, c)
    fine = max(r[1] for r in rows if r[0].startswith("model_fine."))
    coarse = max(r[1] for r in rows if r[0].startswith("model."))
    worst = max(rows, key=lambda r: r[1])
    m, cap = ren.masked_stats[0]
    rgb_err = (rgb.detach().cpu() - c["rgb"]).abs().max().item()
    dep_err = (dep.detach().cpu() - c["depth"]).abs().max().item()
    print(f"masked step [{tag}/{precision}]: loss {loss.item():.8f} (ref {c['loss'].item():.8f}), rgb err {rgb_err:.2e}, depth err {dep_err:.2e}, "
          f"mask bits flipped {n_flipped}, coarse sigma err / range {sig_err:.2e}, M {int(m.item())} of {cap}, "
          f"worst relative gradient error fine {fine:.2e}, coarse {coarse:.2e} ({worst[0]})")
    parity_record("gradients", f"masked_step_vs_reference_autograd/{tag}/{precision}", {
        "loss": loss.item(), "loss_ref": c["loss"].item(), "rgb_max_err": rgb_err, "depth_max_err": dep_err,
        "mask_bits_flipped": n_flipped, "coarse_sigma_err_rel_to_range": sig_err, "points_evaluated": int(m.item()), "capacity": cap,
        "fine_worst_rel_err": fine, "coarse_worst_rel_err": coarse, "worst_tensor": worst[0],
        "per_tensor_rel_err": {k: e for k, e, _ in rows}})
    assert n_flipped == 0
    assert cap == 96 * 192 and int(m.item()) == 64 * 96 + int(c["valid_fine"].sum())
    assert abs(loss.item() - c["loss"].item()) <= 1e-6 * max(1.0, abs(c["loss"].item()))
    assert rgb_err <= 2e-3
    assert fine <= 5e-4 and coarse <= 2.5e-2
    for k in ("model.rgb_linear.weight", "model.views_linears.0.weight", "model.feature_linear.weight"):
        assert torch.all(dict(net.named_parameters())[k].grad == 0), k


# ================================================================================ 2: forward identity
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("tag,family,thr", MASKED_CASES)
def test_masked_forward_under_autograd_equals_the_no_grad_render(amd, family_sd, golden, tag, family, thr, precision):
    """rgb / depth of the masked render under autograd against the no-grad masked render of the same renderer.  The relation
    is the one the UNMASKED pair has, which this test measures first on the same rays: both pairs evaluate every point with
    the same per-point arithmetic (SAVE and inference instances of one kernel, tiles grouped differently), and the unmasked
    pair is bit-equal in both precisions (measured on the MI355X; asserted here, so a change of that relation shows up)."""
    c = _case(golden, tag)
    batch = {"rays_o": c["rays_o"][None].cuda(), "rays_d": c["rays_d"][None].cuda()}
    net = network(amd, family_sd(family), precision, train=True)
    out = {}
    for mode in ("unmasked", "masked"):
        ren = amd.Renderer(net)
        if mode == "masked":
            ren.fast_sampling, ren.weights_threshold = True, thr
        rgb_g, dep_g = ren.render(batch)
        assert rgb_g.requires_grad
        with torch.no_grad():
            rgb_n, dep_n = ren.render(batch)
        assert not rgb_n.requires_grad
        out[mode] = (torch.equal(rgb_g.detach(), rgb_n) and torch.equal(dep_g.detach(), dep_n),
                     (rgb_g.detach() - rgb_n).abs().max().item(), (dep_g.detach() - dep_n).abs().max().item())
        print(f"autograd vs no_grad [{tag}/{precision}/{mode}]: bit-equal {out[mode][0]}, max |d rgb| {out[mode][1]:.2e}, max |d depth| {out[mode][2]:.2e}")
    assert out["unmasked"][0]
    assert out["masked"][0]


# ================================================================================ 3: masked entries against unmasked entries at the ABI
SENTINEL = 12345.0


def _abi_setup(amd, synthetic_sd, precision, n, S, seed):
    L = amd._lib
    net = network(amd, synthetic_sd, precision, train=False)
    prec = L.PRECISIONS[precision]
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3).contiguous().cuda()
    d = torch.randn(n, 3, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous().cuda()
    t = torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, dim=-1).values.cuda().contiguous()
    params = [p.detach().contiguous() for p in net.model_fine.ordered_params()]
    pk_b = torch.empty(int(L.call("nerf_packed_bwd_bytes", prec)), dtype=torch.uint8, device="cuda")
    L.call("nerf_pack_model_bwd", params, pk_b, prec)
    return dict(net=net, prec=prec, gen=gen, o=o, d=d, t=t, params=params, pk_b=pk_b, n=n, S=S, P=n * S, pk=net.packed("fine"))


def _forward(amd, s, entry, index=None, count=None, raw_fill=0.0):
    L, P = amd._lib, s["P"]
    raw = torch.full((s["n"], s["S"], 4), raw_fill, device="cuda")
    save = torch.full((int(L.call("nerf_train_save_floats", P)),), SENTINEL, device="cuda")
    a = (s["o"], s["d"], s["t"], s["S"], s["n"], s["S"])
    if index is None:
        L.call(entry, *a, s["pk"], raw, save, s["prec"])
    else:
        L.call(entry, *a, index, count, s["pk"], raw, save, s["prec"])
    return raw, save


def _backward(amd, s, save, G, index=None, count=None):
    L, P = amd._lib, s["P"]
    gsave = torch.full((int(L.call("nerf_train_grad_floats", P)),), float("nan"), device="cuda")       # rows of dead tiles stay NaN: never read
    g_t = torch.full((s["n"], s["S"]), float("nan"), device="cuda")
    grads = [torch.zeros_like(p) for p in s["params"]]
    a = (s["o"], s["d"], s["t"], s["S"], s["n"], s["S"])
    if index is None:
        L.call("nerf_mlp_backward", *a, s["pk_b"], G, save, gsave, g_t, grads, s["prec"])
    else:
        ws = torch.empty(int(L.call("nerf_mlp_backward_masked_workspace_bytes", P)), dtype=torch.uint8, device="cuda")
        L.call("nerf_mlp_backward_masked", *a, index, count, s["pk_b"], G, save, gsave, g_t, grads, s["prec"], ws)
    torch.cuda.synchronize()
    return g_t, grads


def _compact(amd, s, valid):
    L, P = amd._lib, s["P"]
    index = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.call("nerf_compact_valid_workspace_bytes", P)), dtype=torch.uint8, device="cuda")
    L.call("nerf_compact_valid", valid, P, index, count, ws)
    torch.cuda.synchronize()
    return index, count


@pytest.mark.parametrize("n", [96, 4096])
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_masked_entries_with_every_point_listed_equal_the_unmasked_entries(amd, synthetic_sd, precision, n):
    """index = arange(P) (from nerf_compact_valid on an all-ones mask): `raw`, the whole save buffer (every region, the
    sign-bit blocks, the stamp; rows neither entry writes keep the sentinel) and g_t are bit-equal to
    nerf_mlp_forward_rays_save_for_compositing / nerf_mlp_backward; the parameter gradients equal to the rounding of their
    atomic accumulation order."""
    s = _abi_setup(amd, synthetic_sd, precision, n, 192, seed=41)
    P = s["P"]
    index, count = _compact(amd, s, torch.ones(P, dtype=torch.uint8, device="cuda"))
    assert int(count.item()) == P and torch.equal(index.cpu(), torch.arange(P, dtype=torch.int32))
    raw_u, save_u = _forward(amd, s, "nerf_mlp_forward_rays_save_for_compositing")
    raw_m, save_m = _forward(amd, s, "nerf_mlp_forward_rays_save_masked", index, count)
    torch.cuda.synchronize()
    assert torch.equal(raw_u.view(torch.int32), raw_m.view(torch.int32))
    assert torch.equal(save_u.view(torch.int32), save_m.view(torch.int32))
    G = torch.randn(n, 192, 4, generator=s["gen"]).cuda() * 1e-3 * (raw_u[..., 3:] > 0)     # zero wherever sigma <= 0 (the entries' contract)
    G = G.contiguous()
    gt_u, grads_u = _backward(amd, s, save_u, G)
    gt_m, grads_m = _backward(amd, s, save_m, G, index, count)
    assert torch.isfinite(gt_u).all() and torch.equal(gt_u.view(torch.int32), gt_m.view(torch.int32))
    assert any(g.abs().max() > 0 for g in grads_u)
    assert_grads_equal(grads_m, grads_u)


@pytest.mark.parametrize("n", [96, 4096])
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_masked_entries_on_a_random_half_of_the_points(amd, synthetic_sd, monkeypatch, precision, n):
    """A seeded random half of the ids, M % 32 != 0.  Compaction: the ids ascending, the count.  Forward: rows of listed ids
    against nerf_mlp_forward_rays_save (every tile in full): sigma bit-equal; rgb bit-equal, or exactly 0 where sigma <= 0
    (the for-compositing rule, applied per compact tile); unlisted rows keep the sentinel the test wrote.  Backward: g_t is 0
    at unlisted ids and bit-equal at listed ones, the parameter gradients equal those of nerf_mlp_backward fed the same draw
    with the unlisted rows zeroed.  The same with NERF_DEAD_TILE_SKIP=0 (every occupied compact tile computed)."""
    s = _abi_setup(amd, synthetic_sd, precision, n, 192, seed=43)
    P = s["P"]
    valid = (torch.rand(P, generator=s["gen"]) < 0.5)
    if int(valid.sum()) % 32 == 0:
        valid[int(valid.nonzero()[0])] = False
    M = int(valid.sum())
    assert M % 32 != 0
    ids = valid.nonzero()[:, 0].to(torch.int32)
    valid_d = valid.to(torch.uint8).cuda()
    index, count = _compact(amd, s, valid_d)
    assert int(count.item()) == M and torch.equal(index[:M].cpu(), ids) and torch.all(index[M:] == -7)
    raw_u, save_u = _forward(amd, s, "nerf_mlp_forward_rays_save")
    listed = valid.cuda().view(n, 192)
    G = torch.randn(n, 192, 4, generator=s["gen"]).cuda() * 1e-3 * (raw_u[..., 3:] > 0) * listed[..., None]
    G = G.contiguous()
    gt_u, grads_u = _backward(amd, s, save_u, G)
    for env in ("1", "0"):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        raw_m, save_m = _forward(amd, s, "nerf_mlp_forward_rays_save_masked", index, count, raw_fill=777.0)
        torch.cuda.synchronize()
        assert torch.all(raw_m[~listed] == 777.0)
        ru, rm = raw_u[listed], raw_m[listed]
        assert torch.equal(ru[:, 3].view(torch.int32), rm[:, 3].view(torch.int32))
        same = (ru[:, :3].view(torch.int32) == rm[:, :3].view(torch.int32)).all(dim=1)
        skipped = (rm[:, :3] == 0).all(dim=1) & (ru[:, 3] <= 0)
        assert torch.all(same | skipped)
        if env == "0":
            assert torch.all(same)
        gt_m, grads_m = _backward(amd, s, save_m, G, index, count)
        assert torch.all(gt_m[~listed] == 0)
        assert torch.equal(gt_u[listed].view(torch.int32), gt_m[listed].view(torch.int32))
        assert any(g.abs().max() > 0 for g in grads_u)
        assert_grads_equal(grads_m, grads_u)
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_masked_entries_with_nothing_listed(amd, synthetic_sd, precision):
    """M = 0: success, `raw` and g_t (zero) aside nothing is written, every gradient stays zero.  n_rays = 0: success, nothing
    touched at all.  More than 2^31 - 1 points: refused (point ids are int32)."""
    s = _abi_setup(amd, synthetic_sd, precision, 96, 192, seed=47)
    L, P = amd._lib, s["P"]
    lib, st = L.load(), L.stream_of(s["o"].device)
    index, count = _compact(amd, s, torch.zeros(P, dtype=torch.uint8, device="cuda"))
    assert int(count.item()) == 0 and torch.all(index == -7)
    raw, save = _forward(amd, s, "nerf_mlp_forward_rays_save_masked", index, count, raw_fill=777.0)
    torch.cuda.synchronize()
    assert torch.all(raw == 777.0)
    stamp = int(L.call("nerf_train_save_floats", P)) - 4
    assert torch.all(save[:stamp] == SENTINEL)
    G = torch.randn(96, 192, 4, generator=s["gen"]).cuda().contiguous()
    g_t, grads = _backward(amd, s, save, G, index, count)
    assert torch.all(g_t == 0) and all(torch.all(g == 0) for g in grads)
    # n_rays = 0
    a0 = (s["o"], s["d"], s["t"], 192, 0, 192)
    assert L.call("nerf_mlp_forward_rays_save_masked", *a0, index, count, s["pk"], raw, save, s["prec"]) == 0
    g0 = [torch.zeros_like(p) for p in s["params"]]
    assert L.call("nerf_mlp_backward_masked", *a0, index, count, s["pk_b"], G, save, None, None, g0, s["prec"], None) == 0
    assert lib.nerf_compact_valid(None, 0, None, L.ptr(count, torch.int32), None, st) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and torch.all(raw == 777.0)
    # int32 point ids
    big = (L.ptr(s["o"]), L.ptr(s["d"]), L.ptr(s["t"]), 192, (1 << 31) // 192 + 1, 192)
    assert lib.nerf_mlp_forward_rays_save_masked(*big, L.ptr(index, torch.int32), L.ptr(count, torch.int32), s["pk"].data_ptr(), L.ptr(raw),
                                                 L.ptr(save), s["prec"], st) == -1
    assert lib.nerf_mlp_backward_masked(*big, L.ptr(index, torch.int32), L.ptr(count, torch.int32), s["pk_b"].data_ptr(), L.ptr(G), L.ptr(save),
                                        L.ptr(save), None, L.ptr_array(g0), s["prec"], L.ptr(save), st) == -1
    assert lib.nerf_compact_valid(L.ptr(index, torch.int32), 1 << 31, L.ptr(index, torch.int32), L.ptr(count, torch.int32),
                                  L.ptr(index, torch.int32), st) == -1
    assert lib.nerf_compact_valid_workspace_bytes(1 << 31) == -1 and lib.nerf_mlp_backward_masked_workspace_bytes(1 << 31) == -1


# 256 ids per block, one scan workgroup of 1024 threads over the block counts, ceil(blocks / 1024) consecutive blocks per thread:
# 1023 / 1024 blocks (one per thread), 1025 / 1026 (two per thread: 513 threads busy, the others start past the end, the last
# block ragged), 2050 (three per thread)
@pytest.mark.parametrize("n_points", [1, 255, 256, 257, 256 * 1023, 256 * 1024, 256 * 1024 + 1, 256 * 1025 + 3, 256 * 2049 + 5])
def test_compact_valid_lists_the_set_ids_in_ascending_order(amd, n_points):
    """nerf_compact_valid against numpy.flatnonzero for an empty, a half-set and a full mask: the count, the ids in ascending
    order, and nothing written behind them -- neither in the rest of `index` nor behind the buffer."""
    import numpy as np
    L = amd._lib
    rng = np.random.default_rng(n_points)
    ws_bytes = int(L.call("nerf_compact_valid_workspace_bytes", n_points))
    for density in (0.0, 0.5, 1.0):
        mask = (rng.random(n_points) < density).astype(np.uint8) * rng.integers(1, 256, n_points, dtype=np.uint8)     # any non-zero byte is set
        ref = np.flatnonzero(mask)
        valid = torch.from_numpy(mask).cuda()
        index = torch.full((n_points + 64,), -7, dtype=torch.int32, device="cuda")      # 64 ids of room behind the buffer the entry knows
        count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        L.call("nerf_compact_valid", valid, n_points, index, count, ws)
        torch.cuda.synchronize()
        print(n_points, density, int(count.item()), int(mask.astype(bool).sum()))
        assert int(count.item()) == int((mask != 0).sum()) == ref.size
        got = index.cpu().numpy()
        assert np.array_equal(got[:ref.size], ref)
        assert np.all(got[ref.size:] == -7)
        assert torch.all(ws[ws_bytes:] == 0xA5)


# ================================================================================ 5: dead-tile switch
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("tag,family,thr", MASKED_CASES[:2])
def test_masked_step_same_with_and_without_dead_tile_skipping(amd, family_sd, golden, monkeypatch, tag, family, thr, precision):
    """The masked step against itself with NERF_DEAD_TILE_SKIP=0 (every compact row stored, every occupied compact tile computed):
    rgb / depth / loss bit-identical, all 48 gradients equal to the rounding of their atomic accumulation (form and bound of
    test_training_step_same_with_and_without_dead_tile_skipping)."""
    c = _case(golden, tag)
    out = {}
    for env in ("1", "0"):
        monkeypatch.setenv("NERF_DEAD_TILE_SKIP", env)
        net = network(amd, family_sd(family), precision, train=True)
        ren = amd.Renderer(net)
        ren.fast_sampling, ren.weights_threshold = True, thr
        ren.live_tile_stats, ren.masked_stats = [], []
        rgb, dep = ren.render({"rays_o": c["rays_o"][None].cuda(), "rays_d": c["rays_d"][None].cuda()})
        loss = torch.nn.functional.mse_loss(rgb, c["target"].cuda())
        loss.backward()
        torch.cuda.synchronize()
        st = ren.live_tile_stats[0]
        out[env] = (rgb.detach().clone(), dep.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in net.parameters()],
                    int(st[0].item()), int(ren.masked_stats[0][0].item()))
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP")
    assert all(torch.equal(out["1"][i], out["0"][i]) for i in range(3))
    m = out["1"][5]
    assert out["0"][5] == m and out["0"][4] == (m + 31) // 32 and 0 <= out["1"][4] <= out["0"][4]
    print(f"masked step [{tag}/{precision}]: {out['1'][4]} live of {out['0'][4]} occupied compact tiles ({96 * 192 // 32} tiles unmasked)")
    assert_grads_equal(out["1"][3], out["0"][3])


# ================================================================================ 6: it trains
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_short_masked_training_run_reduces_loss(amd, oracle, family_sd, precision):
    """The loop of test_short_training_run_reduces_loss with fast_sampling (threshold 0.02) on the trained checkpoint, the target
    rendered by the same masked renderer: the fine colour head is knocked off and trained back; same pass condition."""
    from nerf_replication_amd.training import train_step
    torch.manual_seed(0)
    net = network(amd, family_sd("trained"), precision, train=True)
    ren = amd.Renderer(net)
    ren.fast_sampling, ren.weights_threshold = True, 0.02
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
    print(f"masked losses [{precision}]", ["%.5f" % l for l in losses[::4]])
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < 0.25 * losses[0]
    for b, p in zip(before, net.model_fine.pts_linears[3].parameters()):
        assert torch.equal(b, p.detach()) and p.grad is not None


# ================================================================================ 7: coarse-only step
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_coarse_only_step_matches_reference_autograd(amd, family_sd, golden, precision):
    """N_importance = 0 set on the instance, as on the reference's: loss, rgb, depth and the 24 coarse gradients of the fixture;
    the fine sub-model is unused and its .grad stays None.  No sampler is involved, so every tensor is held to the fine-model
    bound of test_training_step_matches_reference_autograd (5e-4 of the tensor's largest entry); depth, which that test does not
    bound, to the 2e-3 that test_render_masked_golden allows the no-grad render."""
    c = _case(golden, "coarse_only")
    net = network(amd, family_sd("trained"), precision, train=True)
    ren = amd.Renderer(net)
    ren.N_importance = 0
    rgb, dep = ren.render({"rays_o": c["rays_o"][None].cuda(), "rays_d": c["rays_d"][None].cuda()})
    assert rgb.requires_grad
    loss = torch.nn.functional.mse_loss(rgb, c["target"].cuda())
    loss.backward()
    torch.cuda.synchronize()
    rows = _grad_rows(net, c, prefixes=("model.",))
    worst = max(rows, key=lambda r: r[1])
    rgb_err = (rgb.detach().cpu() - c["rgb"]).abs().max().item()
    dep_err = (dep.detach().cpu() - c["depth"]).abs().max().item()
    print(f"coarse-only step [{precision}]: loss {loss.item():.8f} (ref {c['loss'].item():.8f}), rgb err {rgb_err:.2e}, depth err {dep_err:.2e}, "
          f"worst relative gradient error {worst[1]:.2e} ({worst[0]})")
    parity_record("gradients", f"coarse_only_step_vs_reference_autograd/{precision}", {
        "loss": loss.item(), "loss_ref": c["loss"].item(), "rgb_max_err": rgb_err, "depth_max_err": dep_err,
        "worst_rel_err": worst[1], "worst_tensor": worst[0], "per_tensor_rel_err": {k: e for k, e, _ in rows}})
    assert len(rows) == 24
    assert abs(loss.item() - c["loss"].item()) <= 1e-6 * max(1.0, abs(c["loss"].item()))
    assert rgb_err <= 2e-3 and dep_err <= 2e-3
    assert worst[1] <= 5e-4
    assert all(p.grad is None for p in net.model_fine.parameters())


# ================================================================================ 8: refusals kept
@pytest.mark.parametrize("mode", ["fast_sampling", "no_importance"])
@pytest.mark.parametrize("precision", ["f16", "f16m32"])
def test_fp16_training_still_refused(amd, synthetic_sd, oracle, precision, mode):
    net = network(amd, synthetic_sd, precision, train=True)
    ren = amd.Renderer(net)
    if mode == "fast_sampling":
        ren.fast_sampling = True
    else:
        ren.N_importance = 0
    o, d = oracle.seeded_rays(32, 3)
    with pytest.raises(NotImplementedError):
        ren.render({"rays_o": o[None].cuda(), "rays_d": d[None].cuda()})
