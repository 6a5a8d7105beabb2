"""CPU tests of tests/ray_side_reference.py, the yardstick of tests/test_gpu_ray_side.py: with the default (CPU float32) exp the
restatement meets the bars the golden-scene tests hold the kernels to, its float64 twins are plain float64 autograd of the oracle's
expressions wherever no decision differs, every edge family reaches the branch it was built for, and for each decision a
deliberately wrong variant shows on the edge sets."""
import functools

import pytest
import torch

import ray_side_reference as RS
from conftest import load_golden

F32 = torch.float32
STRIDES = ((0, 0), (0, "tie"), (64, 0), (0, 128), (64, 128))          # (t stride, u table)


@functools.lru_cache(maxsize=None)
def edge_sampler(ts, us, masks=None, variant=None, seed=0):
    raw, fam = RS.sampler_rays(seed)
    tab = RS.sampler_tables(seed)
    return RS.sample_fine(raw[:, :, 3].contiguous(), tab["t"][ts], tab["u"][us], masks=masks, variant=variant), fam


# ---- the existing bars, with the default callables -------------------------------------------------------------------------------------
def test_sampler_restatement_meets_the_scene_bars(oracle):
    g = load_golden("sampling.npz")
    sig = g["raw_coarse"][:, :, 3].contiguous()
    t_c, u = torch.linspace(2.0, 6.0, 64), torch.linspace(0.0, 1.0, 128)
    out = RS.sample_fine(sig, t_c, u)
    tf, ts = out["t_fine"], out["t_sorted"]
    ref = oracle.fine_sample(torch.relu(sig), t_c.expand(256, 64))
    for want in (g["t_fine"], ref):                                   # test_fine_sampling_stage's bars
        d = (tf - want).abs()
        assert d.max() <= 4.0 / 63 and (d <= 2e-5).float().mean() >= 0.999 and int((d > 1e-3).sum()) <= 33
        assert torch.equal(tf[:, -1], want[:, -1])
    assert torch.equal(ts, torch.sort(torch.cat([g["t_coarse"], tf], 1), dim=-1).values)
    assert (ts - g["t_sorted"]).abs().max() <= 4.0 / 63
    # the sum of the 62 weights is torch.sum's, bit for bit (of the restatement's own weights: torch's CPU cumprod carries the
    # transmittance in float64, the kernels and the restatement in fp32, so the weights agree to rounding only)
    _, w_ref = oracle.transmittance_weights(torch.relu(sig), t_c.expand(256, 64))
    w = out["w"]
    assert (w - w_ref).abs().max() <= 64 * RS.U
    assert torch.equal(out["wsum"], torch.sum(w[:, 1:-1] + 1e-5, -1))
    assert not torch.equal(RS.torch_sum62(w[:, 1:-1] + 1e-5, "sum_ltr"), out["wsum"])


def test_mask_restatement_meets_the_scene_bars(oracle):
    g = load_golden("render_masked.npz")
    sig = g["raw_coarse"][:, :, 3].contiguous()
    t_c, u = torch.linspace(2.0, 6.0, 64), torch.linspace(0.0, 1.0, 128)
    for thr, key in ((0.25, "valid_fine"), (0.02, "valid_fine_thr002")):
        out = RS.sample_fine(sig, t_c, u, masks=(thr, 0.45))
        valid, ts = out["valid_sorted"], out["t_sorted"]
        ref = oracle.fine_valid_mask(torch.relu(sig), t_c.expand(256, 64), weights_threshold=thr)
        for want in (g[key].bool(), ref):                             # test_ess_ert_mask_stage's bars
            n_valid_fine = valid.sum(1) - 64
            assert (n_valid_fine != want.sum(1)).float().mean() <= 0.02
            for r in range(0, 256, 17):
                if n_valid_fine[r] == want[r].sum():
                    kept = torch.sort(torch.cat([t_c, g["t_fine"][r][want[r]]])).values
                    assert (ts[r][valid[r]] - kept).abs().max() <= 4.0 / 63
        # the merged mask is the fine mask carried through the merge, the coarse samples valid
        assert torch.equal(torch.gather(valid, 1, out["slot"]), out["valid_fine"])
        assert torch.equal(valid.sum(1), 64 + out["valid_fine"].sum(1))


def test_composite_restatement_meets_the_scene_bars(oracle):
    g = load_golden("sampling.npz")
    rgb, dep, w = RS.composite(g["raw_fine"], g["t_sorted"], 1)
    ref_rgb, ref_dep = oracle.composite(g["raw_fine"], g["t_sorted"], True)
    assert (w - g["w192"]).abs().max() <= 2e-6                        # test_composite_stage's bars
    assert (rgb - ref_rgb).abs().max() <= 5e-6 and (dep - ref_dep).abs().max() <= 2e-5
    rgb0, dep0, _ = RS.composite(g["raw_coarse"], torch.linspace(2.0, 6.0, 64), 0)
    r0, d0 = oracle.composite(g["raw_coarse"], g["t_coarse"], False)
    assert (rgb0 - r0).abs().max() <= 5e-6 and (dep0 - d0).abs().max() <= 2e-5


# ---- the twins are float64 autograd of the oracle's expressions --------------------------------------------------------------------------
# Both sides are float64 evaluations of one expression that differ in association only, so they differ by the expression's
# conditioning times 2^-53.  The worst conditioned step is the division by denom^2 of a live bin, denom >= 1e-5 by the live rule: an
# amplification of at most 1e10, 1e10 * 2^-53 = 1.1e-6 of a ray's largest gradient.  Compositing has no such step: 192 samples * 2^-53
# * the 1e10 of the last delta bounds it by the same figure.
TWIN_BOUND = 1.2e-6


def _ray_rel(a, b):
    n = a.shape[0]
    a, b = a.reshape(n, -1), b.reshape(n, -1)
    scale = b.abs().amax(dim=1)
    assert bool((a[scale == 0] == 0).all())
    keep = scale > 0
    return ((a[keep] - b[keep]).abs().amax(dim=1) / scale[keep]).max().item() if bool(keep.any()) else 0.0


def plain_sampler_f64(sig, t, u):
    """oracle.fine_sample + cat + torch.sort in float64, every decision made anew -> (t_sorted, parts)."""
    n = sig.shape[0]
    t, u = RS._rows(t, n).double(), RS._rows(u, n).double().contiguous()
    delta = torch.cat([t[:, 1:] - t[:, :-1], 1e10 * torch.ones(n, 1, dtype=torch.float64)], -1)
    alpha = 1.0 - torch.exp(-torch.relu(sig) * delta)
    keep = torch.clamp(1.0 - alpha, min=1e-10, max=1.0)
    T = torch.cumprod(torch.cat([torch.ones(n, 1, dtype=torch.float64), keep], -1), -1)[:, :-1]
    w = (T * alpha)[:, 1:-1] + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cat([torch.zeros(n, 1, dtype=torch.float64), torch.cumsum(pdf, -1)], -1)
    inds = torch.searchsorted(cdf.detach().contiguous(), u, right=True)
    below, above = torch.clamp(inds - 1, 0, 61), torch.clamp(inds, 0, 61)
    bins = 0.5 * (t[:, 1:] + t[:, :-1])
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = ca - cb
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    fine = bb + (u - cb) / denom * (ba - bb)
    order = torch.sort(torch.cat([t, fine], -1), dim=-1, stable=True)
    place = torch.empty_like(order.indices)
    place.scatter_(1, order.indices, torch.arange(192)[None, :].expand(n, 192).contiguous())
    return order.values, {"ind": inds, "live": ~((ca - cb) < 1e-5), "slot": place[:, 64:], "om": 1.0 - alpha}


@pytest.mark.parametrize("ts,us", STRIDES)
def test_sample_twin_is_float64_autograd(ts, us):
    raw, _ = RS.sampler_rays()
    tab = RS.sampler_tables()
    sig, t, u = raw[:, :, 3].contiguous(), tab["t"][ts], tab["u"][us]
    G = torch.randn(RS.N_EDGE, 192, generator=torch.Generator().manual_seed(5))
    # plain autograd hands the cotangents out by torch.sort's own permutation, which orders equal fine depths by position; the kernels
    # and the restatement order them by ascending u.  On ascending u the two coincide, and the merged depths (so their adjoint) depend
    # only on the multiset of u: the comparison runs on each ray's u sorted, and the twin on the caller's order must agree with it.
    u_asc = torch.sort(RS._rows(u, RS.N_EDGE), dim=1).values.contiguous()
    dec = RS.sample_fine(sig, t, u_asc)
    x = sig.double().clone().requires_grad_(True)
    t_sorted, parts = plain_sampler_f64(x, t, u_asc)
    (t_sorted * G.double()).sum().backward()
    same = ((parts["ind"] == dec["ind"]).all(1) & (parts["live"] == dec["live"]).all(1) & (parts["slot"] == dec["slot"]).all(1)
            & (((parts["om"] >= 1e-10) & (parts["om"] <= 1.0)) == dec["passes"]).all(1))
    assert int(same.sum()) >= 8, int(same.sum())           # (u = 1 and 1 - 2^-24 sit on the last cdf value: most edge rays re-decide)
    twin = RS.sample_twin(sig, t, u_asc, G, torch.float64, dec)
    assert _ray_rel(twin[same], x.grad[same]) <= TWIN_BOUND
    own, _ = edge_sampler(ts, us)
    assert _ray_rel(RS.sample_twin(sig, t, u, G, torch.float64, own), twin) <= TWIN_BOUND
    RS.record(f"cpu/sample_twin_rays_compared/t{ts}_u{us}", int(same.sum()))


@pytest.mark.parametrize("S", [2, 17, 64, 192])          # (the oracle's expressions need two samples)
@pytest.mark.parametrize("white", [0, 1])
def test_composite_twin_is_float64_autograd(oracle, S, white):
    raw, t, _ = RS.composite_rays(S)
    gen = torch.Generator().manual_seed(6)
    g_rgb, g_dep = torch.randn(RS.N_EDGE, 3, generator=gen), torch.randn(RS.N_EDGE, generator=gen)
    x, tt = raw.double().clone().requires_grad_(True), t.double().clone().requires_grad_(True)
    rgb, dep = oracle.composite(x, tt, bool(white))
    ((rgb * g_rgb.double()).sum() + (dep * g_dep.double()).sum()).backward()
    om32 = RS.weights(raw[:, :, 3].contiguous(), t)[3]
    delta = torch.cat([tt[:, 1:] - tt[:, :-1], torch.full((RS.N_EDGE, 1), 1e10, dtype=torch.float64)], 1).detach()
    om64 = torch.exp(-torch.relu(x[:, :, 3].detach()) * delta)
    same = (((om64 >= 1e-10) & (om64 <= 1.0)) == RS.pass_mask(om32)).all(1)
    assert int(same.sum()) >= RS.N_EDGE // 2
    g_raw, g_t = RS.composite_twin(raw, t, white, g_rgb, g_dep, torch.float64)
    assert _ray_rel(g_raw[same], x.grad[same]) <= TWIN_BOUND and _ray_rel(g_t[same], tt.grad[same]) <= TWIN_BOUND
    # g_depth = None is a zero cotangent
    a, b = RS.composite_twin(raw, t, white, g_rgb, None, torch.float64)
    a0, b0 = RS.composite_twin(raw, t, white, g_rgb, torch.zeros(RS.N_EDGE), torch.float64)
    assert torch.equal(a, a0) and torch.equal(b, b0)


# ---- non-vacuity -------------------------------------------------------------------------------------------------------------------------
def test_every_family_triggers_its_branch():
    counts = {}
    for ts, us in STRIDES:
        out, fam = edge_sampler(ts, us)
        rows = lambda name: torch.tensor(fam[name])                    # noqa: E731
        c = {"not_live": int((~out["live"]).sum()), "clamp_not_passing": int((~out["passes"]).sum()),
             "T_zero": int((out["T"] == 0).sum()), "T_denormal": int(((out["T"] > 0) & (out["T"] < 1.1754944e-38)).sum()),
             "above_clamped_to_61": int((out["ind"] > 61).sum()), "below_clamped_to_0": int((out["ind"] == 0).sum()),
             "empty_ray": int(out["empty_ray"].sum()), "not_empty_ray": int((~out["empty_ray"]).sum()),
             "object_ray": int(out["object_ray"].sum()), "not_object_ray": int((~out["object_ray"]).sum()),
             "fine_coarse_ties": out["ties"], "inversions_repaired": out["inversions"]}
        for key in ("not_live", "clamp_not_passing", "T_zero", "T_denormal", "above_clamped_to_61", "empty_ray", "not_empty_ray",
                    "object_ray", "not_object_ray"):
            assert c[key] > 0, (ts, us, key)
        # each family, its own branch
        assert bool((out["w"][rows("dead")] == 0).all()) and bool(out["empty_ray"][rows("dead")].all())
        for name in ("one_opaque", "one_opaque_alone"):
            assert bool((~out["passes"][rows(name)]).any(1).all())
        for name in ("five_opaque", "five_opaque_first"):
            assert bool((out["T"][rows(name)] == 0).any(1).all())
        assert bool((~out["passes"][rows("opaque_ends")][:, [0, 63]]).all())
        assert bool((out["w"][rows("tiny")][:, :63] == 0).all()) and bool(out["relu"][rows("tiny")].all())
        assert out["empty_ray"][rows("sum_1e-3")].tolist() == [True, False, False]
        assert out["dsum"][rows("sum_1e-3")][1].item() == torch.tensor(1e-3, dtype=F32).item()
        assert out["object_ray"][rows("max_0.5")].tolist() == [False, False, True, True]
        assert out["dmax"][rows("max_0.5")][:2].tolist() == [0.5, 0.5]
        counts[f"t{ts}_u{us}"] = c
    assert counts["t0_utie"]["fine_coarse_ties"] > 0 and counts["t0_u128"]["fine_coarse_ties"] > 0
    # the masks: each rule decides at least one fine sample on its own
    for masks in RS.MASK_THRESHOLDS:
        out, fam = edge_sampler(0, 0, masks=masks)
        vf = out["valid_fine"]
        counts[f"masks_{masks[0]}_{masks[1]}"] = {"valid_fine": int(vf.sum()), "invalid_fine": int((~vf).sum())}
        assert 0 < int(vf.sum()) < vf.numel()
    out, fam = edge_sampler(0, 0, masks=RS.MASK_THRESHOLDS[2])
    rows = torch.tensor(fam["sum_1e-3"])
    assert out["valid_fine"][rows].all(1).tolist() == [False, True, True]          # the empty-ray test alone, on either side of 1e-3
    out, fam = edge_sampler(0, 0, masks=RS.MASK_THRESHOLDS[1])
    rows = torch.tensor(fam["max_0.5"])
    w_in = out["w"][:, 1:63] < torch.tensor(0.02, dtype=F32)
    differs = torch.gather(w_in, 1, out["below"]) != torch.gather(w_in, 1, out["above"])         # where "and" and "or" part ways
    assert bool(differs[rows[:2]].any()) and bool(differs[rows[2:]].any())
    # ties and inversions: recorded; if the sets hold none, a few more seeds are searched and that is recorded too
    found = {"fine_coarse_ties": sum(c["fine_coarse_ties"] for c in counts.values() if "fine_coarse_ties" in c),
             "inversions_repaired": sum(c["inversions_repaired"] for c in counts.values() if "inversions_repaired" in c)}
    searched = {}
    for key in found:
        if found[key] == 0:
            field = "ties" if key == "fine_coarse_ties" else "inversions"
            searched[key] = {"seeds": [1, 2, 3],
                             "found": sum(edge_sampler(ts, us, seed=s)[0][field] for s in (1, 2, 3) for ts, us in STRIDES)}
    RS.record("cpu/non_vacuity", {"counts": counts, "in_the_sets": found, "searched_further": searched})


def test_composite_families_trigger_their_branches():
    for S in RS.COMPOSITE_S + (193,):
        raw, t, family = RS.composite_rays(S)
        w, T, alpha, om, q = RS.weights(raw[:, :, 3].contiguous(), t)
        fam = lambda name: family == RS.COMPOSITE_FAMILIES.index(name)          # noqa: E731
        assert bool((w[fam("dead")] == 0).all())
        assert bool((~RS.pass_mask(om[fam("one_opaque")])).any(1).all())
        if S >= 6:
            assert bool((T[fam("several_opaque")] == 0).any(1).all())
        if S >= 2:
            assert bool(((t[fam("repeated_depths")][:, 1:] - t[fam("repeated_depths")][:, :-1]) == 0).any(1).all())
        assert bool((raw[fam("rgb_extremes")][:, :, :3].abs() == 100).any()) and (S < 16 or bool((w[fam("semi")] > 0).any(1).all()))
        assert bool((t[:, 1:] >= t[:, :-1]).all())


# ---- discrimination ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["sum_ltr", "clamp62", "left", "fine_first", "last_delta_from_t"])
def test_a_wrong_forward_decision_shows(variant):
    differing = 0
    for ts, us in STRIDES:
        for masks in (None, RS.MASK_THRESHOLDS[1]):
            right, _ = edge_sampler(ts, us, masks=masks)
            wrong, _ = edge_sampler(ts, us, masks=masks, variant=variant)
            if masks and ts + RS.u_stride(us):
                continue                                              # the masks need the shared tables
            keys = ["t_sorted", "t_fine", "slot"] + (["valid_sorted"] if masks else [])
            differing += int(torch.stack([(right[k] != wrong[k]).any(1) for k in keys]).any(0).sum())
    if variant == "last_delta_from_t":
        # the sampler never uses the last sample's weight; compositing does
        assert differing == 0
        raw, t, _ = RS.composite_rays(17)
        right, wrong = RS.composite(raw, t, 1), RS.composite(raw, t, 1, variant=variant)
        differing = int((right[0] != wrong[0]).any(1).sum())
    assert differing > 0
    RS.record(f"cpu/discrimination/{variant}", {"rays_that_differ": differing})


@pytest.mark.parametrize("variant", ["pass_strict", "last_delta_from_t"])
def test_a_wrong_adjoint_decision_shows(variant):
    dec, _ = edge_sampler(0, 0)
    raw, _ = RS.sampler_rays()
    tab = RS.sampler_tables()
    G = torch.randn(RS.N_EDGE, 192, generator=torch.Generator().manual_seed(5))
    sig = raw[:, :, 3].contiguous()
    right = RS.sample_twin(sig, tab["t"][0], tab["u"][0], G, torch.float64, dec)
    wrong = RS.sample_twin(sig, tab["t"][0], tab["u"][0], G, torch.float64, dec, variant=variant)
    n_sampler = int((right != wrong).any(1).sum())
    rawc, t, _ = RS.composite_rays(17)
    gen = torch.Generator().manual_seed(6)
    g_rgb, g_dep = torch.randn(RS.N_EDGE, 3, generator=gen), torch.randn(RS.N_EDGE, generator=gen)
    right = RS.composite_twin(rawc, t, 1, g_rgb, g_dep, torch.float64)
    wrong = RS.composite_twin(rawc, t, 1, g_rgb, g_dep, torch.float64, variant=variant)
    n_comp = int(((right[0] != wrong[0]).any(2).any(1) | (right[1] != wrong[1]).any(1)).sum())
    if variant == "pass_strict":
        assert n_sampler > 0                # 1 - alpha == 1 with sigma > 0: the rays of 1e-30
    assert n_comp > 0
    RS.record(f"cpu/discrimination/adjoint_{variant}", {"sampler_rays_that_differ": n_sampler, "composite_rays_that_differ": n_comp})
