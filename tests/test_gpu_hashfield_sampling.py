"""GPU tests of the hash field's sampling: nerf_field_sample_importance, nerf_field_stratified_depths and
nerf_field_density_scatter bit for bit against the fp32 restatement (tests/hashfield_sampling_reference.py) inside guarded buffers,
then HashRenderer with N_importance / perturb stage by stage through its `samples` hook: the merged depths are the restatement of the
device's own coarse weights, and the weights, the image at the device's depths and the parameter gradients obey the project's rule
against float64,

    max|hip - f64| <= 3 * max|cpu_fp32 - f64| + 2 u max|f64|,   u = 2^-24,

per tensor.  Measured / allowed go to profiles/hashfield_sampling.json."""
import functools

import numpy as np
import pytest
import torch

import hashfield_reference as R
import hashfield_sampling_reference as SR
from gpu_common import Replay, amd  # noqa: F401
from test_gpu_hashfield import (GRID_N, PARAM_KEYS, Guarded, _allowed, batch_of, hand_grid, hip_field, hip_renderer, same,
                                training_field, training_rays)
from test_hashfield_sampling_cpu import COUNTS, depths_of, rays_of_weights, us_of

pytestmark = pytest.mark.gpu


# ---- the entries, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sc,Sf", COUNTS)
def test_sampler_is_the_restatement(amd, Sc, Sf):
    """67 rays (two workgroups, the second with 3 rays): all-zero, one-hot first / last interior, only the two ignored samples,
    1e-30 everywhere and random weights; shared and per-ray coarse depths; a shared ascending u and per-ray unsorted u, both holding
    0, 1 - 2^-24 and 1.  t_fine comes back in the caller's order."""
    n = 67
    w = rays_of_weights(n, Sc, Sc * 1000 + Sf)
    t_tables = {0: torch.linspace(2.0, 6.0, Sc), Sc: depths_of(n, Sc, 5)}
    u_tables = {0: torch.sort(us_of(1, Sf, 6)[0]).values.contiguous(), Sf: us_of(n, Sf, 7)}
    if Sf >= 3:
        assert all(v in u_tables[0].tolist() and v in u_tables[Sf][n - 1].tolist() for v in (0.0, 1.0, 1.0 - 2.0 ** -24))
    for ts, t in t_tables.items():
        for us, u in u_tables.items():
            merged, fine = Guarded((n, Sc + Sf)), Guarded((n, Sf))
            amd._lib.call("nerf_field_sample_importance", w.cuda(), t.cuda(), ts, u.cuda(), us, n, Sc, Sf, merged.view, fine.view)
            want_m, want_f = SR.sample_importance(w, t, u)
            assert same(merged.view, want_m, f"t_merged (t stride {ts}, u stride {us})") and merged.intact()
            assert same(fine.view, want_f, f"t_fine (t stride {ts}, u stride {us})") and fine.intact()
            only = Guarded((n, Sc + Sf))                           # t_fine is optional
            amd._lib.call("nerf_field_sample_importance", w.cuda(), t.cuda(), ts, u.cuda(), us, n, Sc, Sf, only.view, None)
            assert same(only.view, want_m, "t_merged alone") and only.intact()


@pytest.mark.parametrize("S", [1, 2, 3, 64, 192])
def test_stratified_depths_are_the_torch_expression(amd, S):
    n = 65
    t = torch.linspace(2.0, 6.0, S)
    jit = torch.rand(n, S, generator=torch.Generator().manual_seed(S))
    jit[0], jit[1] = 0.0, 1.0 - 2.0 ** -24
    out = Guarded((n, S))
    amd._lib.call("nerf_field_stratified_depths", t.cuda(), jit.cuda(), n, S, out.view)
    assert same(out.view, SR.stratified(t, jit), "t") and out.intact()
    if S == 1:
        assert torch.equal(out.view.cpu(), t.expand(n, 1))


def test_density_scatter_is_the_restatement(amd):
    n_points = 65 * 3
    gen = torch.Generator().manual_seed(1)
    geo = torch.randn(n_points, 16, generator=gen)
    for M in (1, 33, n_points):
        for index in (None, torch.sort(torch.randperm(n_points, generator=gen)[:M]).values.to(torch.int32)):
            raw = Guarded((n_points, 4), fill=0.0)
            amd._lib.call("nerf_field_density_scatter", geo.cuda(), 16, None if index is None else index.cuda(), M, n_points, raw.view)
            assert same(raw.view, SR.density_scatter(geo[:, 0].contiguous(), index, M, n_points), "raw") and raw.intact()
    bad = torch.tensor([0, 5, n_points, -1], dtype=torch.int32)    # an id outside [0, n_points) is never a store address
    raw = Guarded((n_points, 4), fill=0.0)
    amd._lib.call("nerf_field_density_scatter", geo.cuda(), 16, bad.cuda(), 4, n_points, raw.view)
    assert same(raw.view, SR.density_scatter(geo[:, 0].contiguous(), bad[:2], 2, n_points), "raw") and raw.intact()


# ---- the renderer, stage by stage ------------------------------------------------------------------------------------------------------
def importance_renderer(amd, sc, Sc, Sf, requires_grad=False, white=True):
    ren = hip_renderer(amd, hip_field(amd, sc, requires_grad=requires_grad), Sc, white)
    ren.N_importance, ren.samples = Sf, []
    return ren


@functools.lru_cache(maxsize=None)
def staged(Sc):
    """The parity scene with Sc coarse depths, built once."""
    return R.scene(65, Sc)


@pytest.mark.parametrize("Sc,Sf", [(8, 8), (64, 128)])
def test_stages_through_samples(amd, Sc, Sf):
    """The field of the parity test (L=4, T=12, width 64, embeddings U(-0.5, 0.5), 65 rays).  The stages are decoupled through
    `samples`: the sampler is checked on the device's own weights, the image on the device's own depths."""
    sc = staged(Sc)
    ren = importance_renderer(amd, sc, Sc, Sf)
    rgb, depth = ren.render(batch_of(sc))
    assert rgb.shape == (65, 3) and depth.shape == (65,) and not rgb.requires_grad
    assert len(ren.samples) == 1
    t_c, w_c, t_m = ren.samples[0]
    assert t_c.shape == (Sc,) and w_c.shape == (65, Sc) and t_m.shape == (65, Sc + Sf) and t_m.is_cuda
    assert torch.equal(t_c.cpu(), sc["t"])
    want, _ = SR.sample_importance(w_c.cpu(), sc["t"], torch.linspace(0.0, 1.0, Sf))
    assert same(t_m, want, "t_merged")
    figures, ok = {}, []
    t_dev = t_m.cpu()
    res = {}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        params = R.cast_params(sc["params"], dtype)
        with torch.no_grad():
            res[tag] = (SR.coarse_weights(params, sc["o"], sc["d"], sc["t"], sc["frame"], sc["offsets"], sc["scales"]),
                        SR.render_rays(params, sc["o"], sc["d"], t_dev, sc["frame"], 1, sc["offsets"], sc["scales"]))
    assert float(res["f64"][0].max()) > 0.1 and float(res["f64"][1][0].std()) > 1e-3          # weights to sample from; an image
    ok.append(_allowed("weights_coarse", w_c, res["f64"][0], res["cpu32"][0], figures))
    ok.append(_allowed("rgb", rgb, res["f64"][1][0], res["cpu32"][1][0], figures))
    ok.append(_allowed("depth", depth, res["f64"][1][1], res["cpu32"][1][1], figures))
    SR.record(f"stages_{Sc}_{Sf}", figures)
    assert all(ok), figures


def test_parameter_gradients(amd):
    """(8, 8), against float64 autograd with the device's merged depths as constants: the rule above on each of the 11 parameter
    tensors (the gradient rows of DESIGN.md section 2.14's table: "the tensor closest to its bound, of 11"), embedding rows that are
    exactly zero in float64 exactly zero on the device.  Measured: the density head's bias gradient is the closest, 3.47e-06 from
    float64 against an allowance of 3.54e-06 (fp32 on the CPU: 3.42e-07; max |f64| 21, so the device is 2.8 u max|f64| off and
    torch's CPU sum of the same 1040 signed terms 0.3 u); the same figure in two runs.  Every other tensor uses at most 0.75 of
    its allowance."""
    Sc, Sf = 8, 8
    sc = staged(Sc)
    ren = importance_renderer(amd, sc, Sc, Sf, requires_grad=True)
    rgb, depth = ren.render(batch_of(sc))
    assert rgb.requires_grad and depth.requires_grad
    t_c, w_c, t_m = ren.samples[0]
    assert not t_m.requires_grad and not w_c.requires_grad
    gen = torch.Generator().manual_seed(77)
    a, b = torch.randn(65, 3, generator=gen), torch.randn(65, generator=gen)
    ((rgb * a.cuda()).sum() + (depth * b.cuda()).sum()).backward()
    grads = {}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        params = R.cast_params(sc["params"], dtype, requires_grad=True)
        r, z = SR.render_rays(params, sc["o"], sc["d"], t_m.cpu(), sc["frame"], 1, sc["offsets"], sc["scales"])
        ((r * a.to(dtype)).sum() + (z * b.to(dtype)).sum()).backward()
        grads[tag] = [p.grad for p in R.flat_params(params)]
    figures, ok = {}, []
    for name, p, g64, g32 in zip(PARAM_KEYS, ren.field.parameters(), grads["f64"], grads["cpu32"]):
        assert p.grad is not None and p.grad.shape == g64.shape and float(g64.abs().max()) > 0, name
        ok.append(_allowed("grad_" + name, p.grad, g64, g32, figures))
    g_emb, untouched = ren.field.encoder.embeddings.grad.cpu(), grads["f64"][0] == 0
    assert 0 < int(untouched.sum()) < untouched.numel()
    assert bool((g_emb[untouched] == 0).all())
    SR.record("gradients_8_8", figures)
    assert all(ok), [k for k, o in zip(figures, ok) if not o]


def test_coarse_pass_leaves_no_gradient(amd):
    """The proposal is detached.  A field whose COARSE pass alone touches table rows: the sampler's depths are replaced (through the
    renderer's own _depths hook) by depths in the far half of the ray, t in [4.5, 6], while the coarse pass keeps the table over
    [2, 6] -- the rows that only coarse samples in [2, 4] touch get a gradient of exactly zero, and what `samples` hands out carries
    no graph."""
    import hashgrid_reference as H
    Sc, Sf, n = 8, 8, 65
    sc = staged(Sc)
    ren = importance_renderer(amd, sc, Sc, Sf, requires_grad=True)
    far = torch.linspace(4.5, 6.0, Sc + Sf).expand(n, Sc + Sf).contiguous()
    inner = ren._depths

    def far_depths(o, d, table, jitter, u, grid, white):
        t_m, S, stride = inner(o, d, table, jitter, u, grid, white)            # the coarse pass runs, its depths are dropped
        return far.cuda()[:o.shape[0]].contiguous(), S, stride
    ren._depths = far_depths
    rgb, depth = ren.render(batch_of(sc))
    (rgb.sum() + depth.sum()).backward()
    t_c, w_c, t_m = ren.samples[0]
    assert t_m.grad_fn is None and w_c.grad_fn is None and not t_m.requires_grad and not w_c.requires_grad

    def rows_of(x32):
        rows = set()
        for l in range(sc["L"]):
            g, _ = H.cells(x32, sc["scales"][l])
            size = int(sc["offsets"][l + 1] - sc["offsets"][l])
            for idx in range(8):
                rows.update((H.corner_rows(g, idx, size, sc["scales"][l]) + int(sc["offsets"][l])).tolist())
        return rows
    coarse = rows_of(R.points(sc["o"], sc["d"], sc["t"], Sc, None, n * Sc, sc["frame"]))
    fine = rows_of(SR.points_rays(sc["o"], sc["d"], far, None, n * (Sc + Sf), sc["frame"]))
    only_coarse = sorted(coarse - fine)
    assert len(only_coarse) > 0
    g = ren.field.encoder.embeddings.grad.cpu()
    assert bool((g[torch.tensor(only_coarse)] == 0).all()) and float(g.abs().max()) > 0


# ---- identities ------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_untouched_renderer(amd):
    sc = R.scene(65, 64)
    field = hip_field(amd, sc, requires_grad=False)
    plain = hip_renderer(amd, field, 64).render(batch_of(sc))
    ren = hip_renderer(amd, field, 64)
    ren.N_importance, ren.perturb, ren.samples = 0, False, []
    ren._rand = Replay([])                                          # nothing is drawn
    got = ren.render(batch_of(sc))
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and ren.samples == [] and ren._rand.shapes == []
    geo = ren.render_geometry(batch_of(sc))
    assert torch.equal(geo[0], plain[0]) and torch.equal(geo[1], plain[1])


@pytest.mark.parametrize("perturb", [False, True])
def test_chunking_and_seed(amd, perturb):
    """100 rays with chunk_rays 100, 33 and 1: the same bytes, deterministic and with perturb under one seed; another seed, another
    image."""
    sc = R.scene(100, 32)
    ren = importance_renderer(amd, sc, 32, 32)
    ren.perturb = perturb
    results = []
    for chunk in (100, 33, 1):
        ren.chunk_rays = chunk
        torch.manual_seed(5)
        results.append(ren.render(batch_of(sc)))
    for rgb, depth in results[1:]:
        assert torch.equal(rgb, results[0][0]) and torch.equal(depth, results[0][1])
    assert results[0][0].shape == (100, 3) and bool(torch.isfinite(results[0][0]).all())
    ren.chunk_rays = 100
    torch.manual_seed(6)
    other = ren.render(batch_of(sc))
    assert torch.equal(other[0], results[0][0]) != perturb
    ren.N_importance = 0                                            # jitter alone
    if perturb:
        torch.manual_seed(5)
        a = ren.render(batch_of(sc))
        ren.chunk_rays = 33
        torch.manual_seed(5)
        b = ren.render(batch_of(sc))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], results[0][0])


def test_replay_reproduces_the_restatement(amd):
    """Jitter 0.5 everywhere: the coarse depths are the restatement's stratified depths, the merged depths the restatement of the
    device's weights with the replayed u; the draws are [(n, Sc), (n, Sf)], once for all chunks."""
    Sc, Sf, n = 8, 8, 65
    sc = staged(Sc)
    ren = importance_renderer(amd, sc, Sc, Sf)
    ren.perturb, ren.chunk_rays = True, 33
    u = us_of(n, Sf, 3)
    ren._rand = Replay([torch.full((n, Sc), 0.5), u])
    ren.render(batch_of(sc))
    assert ren._rand.shapes == [(n, Sc), (n, Sf)] and len(ren.samples) == 2
    t_c = torch.cat([s[0] for s in ren.samples]).cpu()
    w_c = torch.cat([s[1] for s in ren.samples]).cpu()
    t_m = torch.cat([s[2] for s in ren.samples]).cpu()
    want_c = SR.stratified(sc["t"], torch.full((n, Sc), 0.5))
    assert torch.equal(t_c, want_c)
    assert torch.equal(t_m, SR.sample_importance(w_c, want_c, u)[0])
    ren.N_importance, ren.samples = 0, []                           # without resampling only the jitter is drawn
    ren._rand = Replay([torch.full((n, Sc), 0.5)])
    ren.render(batch_of(sc))
    assert ren._rand.shapes == [(n, Sc)] and ren.samples == []


def test_render_geometry_honours_importance(amd):
    sc = staged(8)
    ren = importance_renderer(amd, sc, 8, 8)
    rgb, depth = ren.render(batch_of(sc))
    ren.geometry_chunk_rays = 33
    g_rgb, g_depth, acc, normal = ren.render_geometry(batch_of(sc))
    assert torch.equal(g_rgb, rgb) and torch.equal(g_depth, depth)
    assert acc.shape == (65,) and normal.shape == (65, 3) and bool(torch.isfinite(normal).all())
    assert bool((normal.norm(dim=1) <= acc + 1e-6).all()) and float(acc.max()) > 0.1
    ren.perturb = True
    with pytest.raises(NotImplementedError):
        ren.render_geometry(batch_of(sc))


def test_ray_gradients_with_the_new_attributes(amd):
    """Rays that require grad: refused with N_importance > 0 before anything is allocated; with jitter alone the per-ray depths are
    constants of the ray adjoint, which runs."""
    sc = staged(8)
    ren = importance_renderer(amd, sc, 8, 8)
    ren.ray_gradients = True
    d = sc["d"].cuda()[None]
    o = sc["o"].cuda()[None].clone().requires_grad_(True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError):
        ren.render({"rays_o": o, "rays_d": d})
    assert torch.cuda.memory_allocated() == before and ren.samples == []
    ren.N_importance, ren.perturb = 0, True
    rgb, _ = ren.render({"rays_o": o, "rays_d": d})
    rgb.sum().backward()
    assert o.grad is not None and bool(torch.isfinite(o.grad).all()) and float(o.grad.abs().max()) > 0


# ---- the grid --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [1, 0])
def test_culling_all_and_nothing(amd, white):
    Sc, Sf = 8, 8
    sc = staged(Sc)
    ren = importance_renderer(amd, sc, Sc, Sf, white=white)
    ren.chunk_rays = 33
    plain = ren.render(batch_of(sc))
    ren.occupancy, ren.stats = hand_grid(amd, np.ones((GRID_N,) * 3, dtype=np.float32)), []
    full = ren.render(batch_of(sc))
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])
    assert ren.stats == [(33 * Sc, 33 * Sc), (33 * (Sc + Sf), 33 * (Sc + Sf)), (32 * Sc, 32 * Sc), (32 * (Sc + Sf), 32 * (Sc + Sf))]
    ren.occupancy, ren.stats = hand_grid(amd, -np.ones((GRID_N,) * 3, dtype=np.float32)), []
    empty = ren.render(batch_of(sc))
    assert torch.equal(empty[0], torch.full((65, 3), float(white), device="cuda")) and torch.equal(empty[1], torch.zeros(65, device="cuda"))
    assert ren.stats == [(0, 33 * Sc), (0, 33 * (Sc + Sf)), (0, 32 * Sc), (0, 32 * (Sc + Sf))]


# ---- training --------------------------------------------------------------------------------------------------------------------------
def run_training(amd, rays, n_samples, n_importance, perturb, steps=40, seed=3):
    """`steps` train_step calls with FusedAdam(lr=1e-2) on the field and the rays of test_gpu_hashfield.test_training_moves."""
    from nerf_replication_amd.training import FusedAdam, train_step
    field = training_field(amd)
    ren = amd.HashRenderer(field)
    ren.N_samples, ren.N_importance, ren.perturb = n_samples, n_importance, perturb
    opt = FusedAdam(field.parameters(), lr=1e-2)
    torch.manual_seed(seed)
    return [float(train_step(ren, opt, *rays)) for _ in range(steps)]


def test_training_moves(amd, oracle, synthetic_sd):
    """40 train_step calls on the setting of test_gpu_hashfield.test_training_moves with 32 + 32 samples and perturb, against the
    uniform 64-sample path from the same state: the loss falls, and ends at most k times where the uniform path ends.  k is twice the
    largest ratio (any importance run over any uniform run) in five runs of each side, made by tools/measure_hashfield_sampling_k.py
    and kept in profiles/hashfield_sampling.json under "training_k"; the test reads it from there."""
    rec = SR.read_record().get("training_k")
    assert rec is not None and rec["k"] == 2.0 * rec["largest_ratio"], "run tools/measure_hashfield_sampling_k.py"
    k = rec["k"]
    rays = training_rays(amd, oracle, synthetic_sd)
    sampled = run_training(amd, rays, 32, 32, True)
    uniform = run_training(amd, rays, 64, 0, False)
    print(f"32 + 32 perturb {sampled[0]:.5f} -> {sampled[-1]:.5f}   uniform 64 {uniform[0]:.5f} -> {uniform[-1]:.5f}   "
          f"ratio {sampled[-1] / uniform[-1]:.3f}   k {k:.5f}")
    SR.record("training_moves", {"importance_first": sampled[0], "importance_last": sampled[-1], "uniform_first": uniform[0],
                                 "uniform_last": uniform[-1], "k": k})
    assert sampled[-1] < sampled[0] and uniform[-1] < uniform[0]
    assert sampled[-1] <= k * uniform[-1]
