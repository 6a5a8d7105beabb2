"""GPU tests of training with an occupancy grid: nerf_occupancy_age against the NumPy restatement
tests/occupancy_train_reference.py (byte for byte), OccupancyGrid.refresh against fresh builds, and the culled training step
(Renderer.train_occupancy) against the plain step: outputs bit-equal and gradients equal to the rounding of their accumulation
order on every ray none of whose culled fine samples has a positive density, which the staged plain entries decide."""
import functools

import numpy as np
import pytest
import torch

import isosurface_reference as R
import occupancy_reference as O
import occupancy_train_reference as A
from conftest import parity_record
from gpu_common import Replay, amd, assert_grads_equal, network, rel  # noqa: F401

pytestmark = pytest.mark.gpu

BOX = [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0]
BIG_BOX = [-8.0, -8.0, -8.0, 8.0, 8.0, 8.0]          # contains every sample: |o| = 4.03, t <= 6
N_PROBE = 512
SENTINEL_F, SENTINEL_B, PAD = 12345.0, 77, 6


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the age kernel --------------------------------------------------------------------------------------------------------------
def _age_abi(amd, field, stride, n, level, hold, age_buf, on_buf):
    L = amd._lib
    L.call("nerf_occupancy_age", L.strided(field), stride, n, level, hold, age_buf, on_buf)
    torch.cuda.synchronize()


@pytest.mark.parametrize("hold", [1, 2, 3])
@pytest.mark.parametrize("shape", [(9, 12, 17), (33, 33, 33)], ids=lambda s: "x".join(map(str, s)))
def test_age_equals_the_restatement(amd, shape, hold):
    """Three successive fields (torus, sphere, torus at another level, one NaN point each) through one age state: age and `on` equal
    the restatement's bytes after every call, dense (stride 1) and as the sigma column of a raw buffer (stride 4, NaN in the channels
    that must not be read), the bytes behind both buffers stay untouched, and `on` aliased to the field gives the same bytes.
    1836 points are no multiple of the 256-thread block, 35 937 take more than one block.  The bitfield built from `on` is the union
    of the direct builds of the last `hold` fields."""
    L = amd._lib
    n = shape[0] * shape[1] * shape[2]
    steps = [("torus", 0.0), ("sphere", 0.0), ("torus", -0.25)]
    ref_age = {s: A.new_age(n) for s in (1, 4)}
    age_buf = {s: torch.full((n + PAD,), SENTINEL_B, dtype=torch.uint8, device="cuda") for s in (1, 4, "alias")}
    for b in age_buf.values():
        b[:n] = 255
    direct = []
    for i, (name, level) in enumerate(steps):
        f = np.array(R.analytic_field(name, shape))
        f[tuple((m // 3 + i) % m for m in shape)] = np.nan
        direct.append(O.build(f, level, 1))
        for stride in (1, 4):
            ref_age[stride], ref_on = A.age_step(f, level, hold, ref_age[stride])
            if stride == 1:
                field = torch.from_numpy(f).cuda()
            else:
                raw = torch.full(shape + (4,), float("nan"), device="cuda")
                raw[..., 3] = torch.from_numpy(f).cuda()
                field = raw[..., 3]
            assert field.stride(2) == stride
            on_buf = torch.full((n + PAD,), SENTINEL_F, device="cuda")
            _age_abi(amd, field, stride, n, level, hold, age_buf[stride], on_buf)
            assert (age_buf[stride][n:] == SENTINEL_B).all() and (on_buf[n:] == SENTINEL_F).all()
            assert np.array_equal(age_buf[stride][:n].cpu().numpy(), ref_age[stride]), (name, stride)
            assert np.array_equal(on_buf[:n].cpu().numpy().view(np.uint32), ref_on.view(np.uint32)), (name, stride)
            if stride == 4:
                assert torch.isnan(raw[..., :3]).all() and np.array_equal(raw[..., 3].cpu().numpy().view(np.uint32), f.view(np.uint32))
        # `on` aliased to the field
        field = torch.full((n + PAD,), SENTINEL_F, device="cuda")
        field[:n] = torch.from_numpy(f).cuda().reshape(-1)
        _age_abi(amd, field, 1, n, level, hold, age_buf["alias"], field)
        assert (field[n:] == SENTINEL_F).all() and (age_buf["alias"][n:] == SENTINEL_B).all()
        assert np.array_equal(field[:n].cpu().numpy().view(np.uint32), ref_on.view(np.uint32))
        assert np.array_equal(age_buf["alias"][:n].cpu().numpy(), ref_age[1])
        # the bitfield of `on`: the OR of the direct builds of the last `hold` fields
        n_words = int(L.call("nerf_occupancy_words", *shape))
        bits = torch.empty(n_words, dtype=torch.int32, device="cuda")
        L.call("nerf_occupancy_build", field, 1, *shape, 0.0, 1, bits)
        torch.cuda.synchronize()
        union = functools.reduce(np.bitwise_or, direct[max(0, i - hold + 1):i + 1])
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), union), (name, hold)
    assert 0 < int((torch.from_numpy(ref_age[1]) == 0).sum()) < n               # neither everything hit nor nothing


# ---- shared pieces ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probe_rays():
    """The 512 probe rays of the occupancy render tests: seeded pixels of the 40-degree pose."""
    import nerf_oracle
    ids = torch.from_numpy(np.random.default_rng(5).choice(800 * 800, N_PROBE, replace=False))
    o, d = nerf_oracle.pinhole_rays(800, 800, nerf_oracle.camera_pose(40.0), pixel_ids=ids)
    return o.cuda(), d.cuda()


def _mark(amd, grid, o, d, t_sorted):
    n = o.shape[0]
    valid = torch.empty(n, 192, dtype=torch.uint8, device="cuda")
    amd._lib.call("nerf_occupancy_mark", o, d, t_sorted, 192, n, 192, grid.bits["fine"], *grid.lookup_args(), 0, valid)
    torch.cuda.synchronize()
    return valid.bool()


def _fine_raw(amd, net, o, d, t_sorted):
    """The plain fine pass of the staged entries on given merged depths -> raw [n,192,4]."""
    L = amd._lib
    n = o.shape[0]
    raw_f = torch.empty(n, 192, 4, device="cuda")
    L.call("nerf_mlp_forward_rays", o, d, t_sorted, 192, n, 192, net.packed("fine"), raw_f, L.PRECISIONS[net.precision])
    return raw_f


def _step(amd, net, o, d, target, grid=None, fast=None, draws=None, every=16):
    """One training step without the optimizer (render, MSE, backward) -> dict of detached results.  grid: Renderer.train_occupancy;
    fast: weights_threshold of fast_sampling; draws: (jitter, u) replayed through Renderer._rand in training sampling mode."""
    for p in net.parameters():
        p.grad = None
    ren = amd.Renderer(net)
    assert ren.occupancy is None
    ren.train_occupancy, ren.train_occupancy_every = grid, every
    if fast is not None:
        ren.fast_sampling, ren.weights_threshold = True, fast
    if draws is not None:
        ren.task, ren.perturb = "train", True
        ren._rand = Replay(draws)
    ren.masked_stats, ren.live_tile_stats, ren.capture_adjoints = [], [], {}
    rgb, dep = ren.render({"rays_o": o[None], "rays_d": d[None]})
    assert rgb.requires_grad
    loss = torch.nn.functional.mse_loss(rgb, target)
    loss.backward()
    torch.cuda.synchronize()
    assert draws is None or not ren._rand.draws
    grads = [p.grad.detach().clone() for p in net.parameters()]
    assert len(grads) == 48
    count = None
    if ren.masked_stats:
        (m, cap), = ren.masked_stats
        assert cap == 192 * o.shape[0] and m.is_cuda
        count = int(m.item())
    return dict(rgb=rgb.detach().clone(), depth=dep.detach().clone(), loss=loss.detach().clone(), grads=grads, count=count,
                cap=ren.capture_adjoints, tiles=ren.live_tile_stats)


def _target(n, seed):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)).cuda()


# ---- 2. refresh ---------------------------------------------------------------------------------------------------------------------
def _perturb_fine(net, seed):
    """An in-place update of the fine model's density head and of a trunk layer: 3 % of each tensor's spread, which moves dozens of
    the 1408 cells of the (9,12,17) grid in and out (CPU probe with the oracle's network: 37 to 213 cells per update)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in (net.model_fine.alpha_linear.weight, net.model_fine.pts_linears[7].weight):
            p.add_((0.03 * float(p.std()) * torch.randn(p.shape, generator=g)).to(p.device))


def test_refresh(amd, family_sd):
    dims = (9, 12, 17)
    net = network(amd, family_sd("sharp"), "f32", train=False)
    grid = amd.OccupancyGrid.from_network(net, BOX, dims, dilate=0)
    assert grid.hold == 1 and grid.uses == 0 and not grid.stale(net, "fine")
    coarse, ptr, words = grid.bits[""].clone(), grid.bits["fine"].data_ptr(), grid.bits["fine"].numel()
    before = grid.bits["fine"].clone()
    _perturb_fine(net, 1)
    assert grid.stale(net, "fine") and not grid.stale(net, "")
    grid.uses = 7
    grid.refresh(net, models=("fine",))
    fresh = amd.OccupancyGrid.from_network(net, BOX, dims, dilate=0, models=("fine",))
    assert torch.equal(grid.bits["fine"], fresh.bits["fine"]) and not torch.equal(before, fresh.bits["fine"])
    assert grid.bits["fine"].data_ptr() == ptr and grid.bits["fine"].numel() == words
    assert not grid.stale(net, "fine") and grid.uses == 0
    assert torch.equal(grid.bits[""], coarse)
    grid.refresh(net)                                                     # default: every model the grid has; nothing moved
    assert torch.equal(grid.bits["fine"], fresh.bits["fine"]) and torch.equal(grid.bits[""], coarse)
    # hold = 2: the OR of the last two direct builds; the build that created the grid is not remembered
    grid = amd.OccupancyGrid.from_network(net, BOX, dims, dilate=0, models=("fine",))
    grid.hold = 2
    builds = []
    for k, seed in enumerate((2, 3, 4)):
        _perturb_fine(net, seed)
        builds.append(amd.OccupancyGrid.from_network(net, BOX, dims, dilate=0, models=("fine",)).bits["fine"])
        grid.refresh(net)
        want = builds[k] if k == 0 else builds[k - 1] | builds[k]
        assert torch.equal(grid.bits["fine"], want), k
        assert not grid.stale(net, "fine")
    assert not torch.equal(builds[0], builds[1]) and not torch.equal(builds[1], builds[2])
    assert any(not torch.equal(builds[k - 1] | builds[k], builds[k]) for k in (1, 2))       # a union that is more than its last build
    # a grid from fields can be refreshed too, and then carries a key
    fields = amd.OccupancyGrid.from_fields(BOX, fine=torch.ones(dims, device="cuda"), dilate=0)
    assert fields.keys is None and fields.occupied_fraction("fine") == 1.0
    fields.refresh(net)
    assert torch.equal(fields.bits["fine"], builds[2]) and not fields.stale(net, "fine")
    _perturb_fine(net, 5)
    assert fields.stale(net, "fine")


# ---- 3. the culled step is the plain step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x"])
@pytest.mark.parametrize("family", ["trained", "sharp"])
def test_culled_step_is_the_plain_step(amd, family_sd, family, precision):
    """Grid N = 64, dilate 1 on [-2,2]^3, the 512 probe rays.  The staged plain entries decide which rays have a culled FINE sample
    with sigma > 0; those are left out, and they may be at most 2 % of the 512 (a condition: the CPU probe with the oracle's grid gives
    3 / 512 on trained, 0 / 512 on sharp; the margin is for last-bit differences between the GPU grid and the oracle's).  On the
    others: rgb, depth and the loss bit-equal, the list is the mark of the selected rays and at most half of the points (probe: 0.21
    and 0.335), all 48 gradients within 1e-4 of the tensor's maximum, exact zeros where the plain step has zeros."""
    L = amd._lib
    net = network(amd, family_sd(family), precision, train=True)
    o, d = _probe_rays()
    n, prec = N_PROBE, L.PRECISIONS[precision]
    grid = amd.OccupancyGrid.from_network(net, BOX, 64, dilate=1, models=("fine",))
    t_c, u = torch.linspace(2.0, 6.0, 64).cuda(), torch.linspace(0.0, 1.0, 128).cuda()
    raw_c = torch.empty(n, 64, 4, device="cuda")
    L.call("nerf_mlp_forward_rays_density", o, d, t_c, 0, n, 64, net.packed(""), raw_c, prec)
    t_sorted = torch.empty(n, 192, device="cuda")
    L.call("nerf_sample_fine", raw_c, t_c, u, n, t_sorted, None, None, 0.0, 0.0)
    raw_f = _fine_raw(amd, net, o, d, t_sorted)
    keep_f = _mark(amd, grid, o, d, t_sorted)
    excluded = (~keep_f & (raw_f[..., 3] > 0)).any(1)
    n_ex = int(excluded.sum())
    print(family, precision, "excluded rays", n_ex, "culled fine samples with sigma > 0", int((~keep_f & (raw_f[..., 3] > 0)).sum()))
    assert n_ex <= 0.02 * n
    sel = ~excluded
    o_s, d_s = o[sel].contiguous(), d[sel].contiguous()
    m = o_s.shape[0]
    target = _target(m, 17)
    plain = _step(amd, net, o_s, d_s, target)
    culled = _step(amd, net, o_s, d_s, target, grid=grid)
    assert plain["count"] is None and grid.uses == 1 and not grid.stale(net, "fine")
    assert torch.equal(culled["cap"]["valid_sorted"].bool(), keep_f[sel])
    d_rgb = (culled["rgb"] - plain["rgb"]).abs().max().item()
    d_dep = (culled["depth"] - plain["depth"]).abs().max().item()
    rels = [(rel(a, b) if b.abs().max() > 0 else float(a.abs().max())) for a, b in zip(culled["grads"], plain["grads"])]
    stats = dict(excluded_rays=n_ex, n_rays=n, selected_rays=m, share_evaluated=culled["count"] / (192 * m), rgb_max_diff=d_rgb,
                 depth_max_diff=d_dep, loss_plain=plain["loss"].item(), loss_culled=culled["loss"].item(),
                 worst_rel_gradient_diff=max(rels), per_tensor_rel_diff=rels,
                 live_tiles_fine_plain=int(plain["tiles"][0][0].item()), live_tiles_fine_culled=int(culled["tiles"][0][0].item()))
    print(family, precision, {k: v for k, v in stats.items() if k != "per_tensor_rel_diff"})
    parity_record("occupancy_train_vs_plain_step", f"{family}/{precision}/N64_dilate1", stats)
    assert _same_bits(culled["rgb"], plain["rgb"]) and _same_bits(culled["depth"], plain["depth"])
    assert _same_bits(culled["loss"].reshape(1), plain["loss"].reshape(1))
    assert culled["count"] == int(keep_f[sel].sum())
    assert culled["count"] <= 0.5 * 192 * m
    assert any(g.abs().max() > 0 for g in plain["grads"][24:])
    assert_grads_equal(culled["grads"], plain["grads"])


# ---- 4. degenerate grids ------------------------------------------------------------------------------------------------------------
def _draws(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 64, generator=g), torch.rand(n, 128, generator=g)


@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_all_occupied_and_all_empty_grids(amd, family_sd, precision):
    n = 96
    net = network(amd, family_sd("sharp"), precision, train=True)
    o, d = (x[:n].contiguous() for x in _probe_rays())
    target = _target(n, 19)
    ones = torch.ones(5, 6, 7, device="cuda")
    full = amd.OccupancyGrid.from_fields(BIG_BOX, fine=ones)
    empty = amd.OccupancyGrid.from_fields(BIG_BOX, fine=-ones)
    assert full.occupied_fraction("fine") == 1.0 and empty.occupied_fraction("fine") == 0.0

    def same(got, ref):
        assert _same_bits(got["rgb"], ref["rgb"]) and _same_bits(got["depth"], ref["depth"])
        assert _same_bits(got["loss"].reshape(1), ref["loss"].reshape(1))
        assert_grads_equal(got["grads"], ref["grads"])

    # every cell occupied: the plain step on a list of all the points
    got = _step(amd, net, o, d, target, grid=full)
    assert got["count"] == 192 * n
    same(got, _step(amd, net, o, d, target))
    # with fast_sampling the sampler's mask alone decides: the masked step
    ref = _step(amd, net, o, d, target, fast=0.02)
    got = _step(amd, net, o, d, target, grid=full, fast=0.02)
    assert got["count"] == ref["count"] and 64 * n <= got["count"] < 192 * n
    assert torch.equal(got["cap"]["valid_sorted"], ref["cap"]["valid_sorted"])
    same(got, ref)
    # stochastic sampling, the same draws
    ref = _step(amd, net, o, d, target, draws=_draws(n, 23))
    got = _step(amd, net, o, d, target, grid=full, draws=_draws(n, 23))
    assert got["count"] == 192 * n and torch.equal(got["cap"]["t_sorted"], ref["cap"]["t_sorted"])
    assert not torch.equal(got["cap"]["t_sorted"], _step(amd, net, o, d, target)["cap"]["t_sorted"])      # the draws were used
    same(got, ref)
    # nothing evaluated: the white background, depth 0, no gradient at all
    for kw in (dict(), dict(fast=0.02), dict(draws=_draws(n, 23))):
        got = _step(amd, net, o, d, target, grid=empty, **kw)
        assert got["count"] == 0
        assert (got["rgb"] == 1.0).all() and (got["depth"] == 0.0).all()
        for i, g in enumerate(got["grads"]):
            assert torch.isfinite(g).all() and torch.all(g == 0), (kw.keys(), i)
    assert full.uses == 3 and empty.uses == 3                             # grids from fields: counted, never refreshed


# ---- 5. stochastic sampling with a real grid -------------------------------------------------------------------------------------------
def test_stochastic_step_with_a_grid(amd, family_sd):
    """Trained, f32, 96 rays, replayed draws.  The coarse pass is not culled, so the merged depths are the plain stochastic step's;
    the list is the mark of the step's own depths; rays the grid keeps whole, and rays none of whose culled samples has a positive
    density (decided by the plain fine pass of the staged entries on the step's depths), have the plain step's rgb bit for bit."""
    n = 96
    net = network(amd, family_sd("trained"), "f32", train=True)
    o, d = (x[:n].contiguous() for x in _probe_rays())
    target = _target(n, 29)
    grid = amd.OccupancyGrid.from_network(net, BOX, 64, dilate=1, models=("fine",))
    plain = _step(amd, net, o, d, target, draws=_draws(n, 31))
    got = _step(amd, net, o, d, target, grid=grid, draws=_draws(n, 31))
    assert torch.isfinite(got["rgb"]).all() and torch.isfinite(got["depth"]).all() and torch.isfinite(got["loss"])
    assert all(torch.isfinite(g).all() for g in got["grads"])
    t_sorted = got["cap"]["t_sorted"]
    assert torch.equal(t_sorted, plain["cap"]["t_sorted"])
    keep = _mark(amd, grid, o, d, t_sorted)
    assert got["count"] == int(keep.sum()) and torch.equal(got["cap"]["valid_sorted"].bool(), keep)
    assert 0 < got["count"] < 192 * n
    whole = keep.all(1)
    assert _same_bits(got["rgb"][whole], plain["rgb"][whole]) and _same_bits(got["depth"][whole], plain["depth"][whole])
    raw_f = _fine_raw(amd, net, o, d, t_sorted)
    exact = ~(~keep & (raw_f[..., 3] > 0)).any(1)
    print("stochastic step with a grid: share evaluated", got["count"] / (192 * n), "rays kept whole", int(whole.sum()),
          "rays without a culled positive density", int(exact.sum()), "of", n)
    assert exact.sum() >= n // 2                                           # the comparison says something
    assert _same_bits(got["rgb"][exact], plain["rgb"][exact]) and _same_bits(got["depth"][exact], plain["depth"][exact])


# ---- 6. it trains -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_short_culled_training_run_reduces_loss(amd, oracle, family_sd, precision):
    """The loop of test_short_masked_training_run_reduces_loss with Renderer.train_occupancy (N = 64, every 4, hold 2) on the trained
    checkpoint: the fine colour head is knocked off and trained back; same pass condition.  25 steps whose parameters all moved,
    one build per 4 steps: refreshes before steps 5, 9, 13, 17, 21 and 25."""
    from nerf_replication_amd.training import train_step
    torch.manual_seed(0)
    net = network(amd, family_sd("trained"), precision, train=True)
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
    grid = amd.OccupancyGrid.from_network(net, BOX, 64, dilate=1, models=("fine",))
    grid.hold = 2
    ren.train_occupancy, ren.train_occupancy_every = grid, 4
    ren.masked_stats = []
    refreshes, refresh = [], grid.refresh

    def counted(*a, **k):
        refreshes.append(len(ren.masked_stats) + 1)                       # the step it comes before
        return refresh(*a, **k)
    grid.refresh = counted
    head = list(net.model_fine.rgb_linear.parameters())
    opt = torch.optim.Adam(head, lr=2e-2, eps=1e-8)
    before = [p.detach().clone() for p in net.model_fine.pts_linears[3].parameters()]
    losses = [train_step(ren, opt, o, d, target).item() for _ in range(25)]
    shares = [int(m.item()) / cap for m, cap in ren.masked_stats]
    print(f"culled losses [{precision}]", ["%.5f" % l for l in losses[::4]], "share evaluated %.3f .. %.3f" % (min(shares), max(shares)),
          "refreshes before steps", refreshes)
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < 0.25 * losses[0]
    assert refreshes == [5, 9, 13, 17, 21, 25]
    assert len(shares) == 25 and max(shares) < 1.0
    assert ren.occupancy is None
    for b, p in zip(before, net.model_fine.pts_linears[3].parameters()):
        assert torch.equal(b, p.detach()) and p.grad is not None


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(amd, family_sd):
    o, d = (x[:64].contiguous() for x in _probe_rays())
    net = network(amd, family_sd("sharp"), "f32", train=True)
    grid = amd.OccupancyGrid.from_network(net, BOX, (9, 12, 17), models=("fine",))
    r = amd.Renderer(net)
    r.train_occupancy = grid
    r.masked_stats = []
    batch = {"rays_o": o[None], "rays_d": d[None]}

    def refused(exc, b=batch):
        with pytest.raises(exc):
            r.render(b)
        assert r.masked_stats == [] and grid.uses == 0                    # nothing ran, nothing counted

    refused(NotImplementedError, b={"rays_o": o[None].clone().requires_grad_(True), "rays_d": d[None]})
    r.N_importance = 0
    refused(NotImplementedError)
    r.N_importance = 128
    for precision in ("f16", "f16m32"):
        net.precision = precision
        refused(NotImplementedError)
    net.precision = "f32"
    r.fast_sampling, r.task = True, "train"
    refused(NotImplementedError)
    r.fast_sampling, r.task = False, "test"
    r.train_occupancy = amd.OccupancyGrid.from_network(net, BOX, (9, 12, 17), models=("",))
    refused(ValueError)
    r.train_occupancy = "grid"
    refused(TypeError)
    r.train_occupancy, r.train_occupancy_every = grid, 0
    refused(ValueError)
    r.train_occupancy_every = 16
    # under no_grad / eval() the attribute changes no bit of the render
    plain = amd.Renderer(net)
    for mode in ("no_grad", "eval"):
        if mode == "eval":
            net.eval()
        with torch.no_grad() if mode == "no_grad" else torch.enable_grad():
            rgb0, dep0 = plain.render(batch)
            rgb1, dep1 = r.render(batch)
        assert not rgb1.requires_grad and _same_bits(rgb1, rgb0) and _same_bits(dep1, dep0)
    assert r.masked_stats == [] and grid.uses == 0
    net.train()
    rgb, _ = r.render(batch)                                              # and the step itself runs
    assert rgb.requires_grad and len(r.masked_stats) == 1 and grid.uses == 1
    torch.cuda.synchronize()
