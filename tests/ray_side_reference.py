"""Restatement of the NeRF path's ray side (include/nerf_mi355x.h: nerf_sample_fine / nerf_sample_fine_rays, nerf_composite and the two
adjoints), in torch on the CPU: the yardstick of tests/test_ray_side_reference_cpu.py and tests/test_gpu_ray_side.py.  A helper, not a
test; written from the header's formulas and the kernels' documented order, and it imports nothing of the package.

    fp32, the documented order  weights, sample_fine, composite: every operation one separately rounded torch op, every sum sequential
                                in the documented order, so the forward kernels match them bit for bit.  The only ingredient that is
                                not IEEE arithmetic is exp: `alpha_of(sigma, delta)` and `sigmoid(x)` are injected callables (defaults:
                                CPU float32); the GPU tests inject lookups of the device's own values.
    the adjoints                composite_twin, sample_twin: differentiable torch in float64 or float32 that takes every discrete
                                decision (relu mask, clamp-pass mask, bins, live, merged slot, the fixed last delta) from the fp32
                                restatement and everything smooth from the dtype in use.
    edge rays                   sampler_rays, sampler_tables, composite_rays: the seeded sets both test modules run on.

`variant` names one deliberately wrong decision (tests of discrimination only): "sum_ltr", "clamp62", "left", "fine_first", "pass_strict",
"last_delta_from_t"."""
import json
import os
import shutil

import numpy as np
import torch

U = 2.0 ** -24
EPS_W = 1e-5
N_SAMPLES, N_IMPORTANCE = 64, 128
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_SIDE_JSON = os.path.join(REPO, "profiles", "ray_side.json")
GOLDEN = os.path.join(REPO, "tests", "golden")
F32 = torch.float32
MASK_THRESHOLDS = ((0.25, 0.45),     # the renderer's defaults
                   (0.02, 0.45),     # the pair test_ess_ert_mask_stage adds
                   (0.0, 0.45))      # no weight is below 0: the only pair under which the empty-ray test alone decides a ray of small densities


def f32(x):
    return torch.tensor(x, dtype=F32)


def div_rn(a, b):
    """The correctly rounded fp32 quotient (through float64: 53 >= 2 * 24 + 2 bits, so the second rounding is innocuous)."""
    return (a.double() / b.double()).to(a.dtype)


def alpha_default(sigma, delta):
    return 1.0 - torch.exp(-sigma * delta)


def sigmoid_default(x):
    return div_rn(torch.ones_like(x), 1.0 + torch.exp(-x))


def _rows(x, n):
    return x[None, :].expand(n, x.shape[0]) if x.dim() == 1 else x


def deltas(t, variant=None):
    """t [n,S] -> delta [n,S]: fsub(t[k + 1], t[k]), the last one 1e10."""
    last = torch.full_like(t[:, :1], 1e10)
    if variant == "last_delta_from_t" and t.shape[1] > 1:
        last = t[:, -1:] - t[:, -2:-1]
    return torch.cat([t[:, 1:] - t[:, :-1], last], dim=1)


# ---- fp32 restatements -----------------------------------------------------------------------------------------------------------------
def weights(sigma, t, alpha_of=alpha_default, variant=None):
    """sigma [n,S] (pre-ReLU), t [n,S] float32 -> (w, T, alpha, om, q), each [n,S]: alpha of relu(sigma) over delta, om = fsub(1, alpha),
    q = clamp(om, 1e-10, 1), T the sequential product T = fmul(T, q) from 1, w = fmul(T, alpha)."""
    assert sigma.dtype == t.dtype == F32
    n, S = sigma.shape
    alpha = alpha_of(torch.clamp_min(sigma, 0.0), deltas(t, variant))
    assert alpha.dtype == F32
    om = 1.0 - alpha
    q = torch.clamp(om, min=1e-10, max=1.0)
    T = torch.ones(n, S, dtype=F32)
    for k in range(1, S):
        T[:, k] = T[:, k - 1] * q[:, k - 1]
    return T * alpha, T, alpha, om, q


def torch_sum62(x, variant=None):
    """torch.sum over 62 fp32 elements in the CPU kernel's order: the 56 leading ones as 7 vectors of 8 with lane sums in the order
    v0, v4, v5, v6, v1, v2, v3, then the 6 tail elements one by one, then the 8 lane sums."""
    assert x.shape[1] == 62 and x.dtype == F32
    if variant == "sum_ltr":
        acc = x[:, 0].clone()
        for k in range(1, 62):
            acc = acc + x[:, k]
        return acc
    v = [x[:, 8 * i:8 * i + 8] for i in range(7)]
    P = v[0] + v[4]
    for i in (5, 6, 1, 2, 3):
        P = P + v[i]
    acc = x[:, 56].clone()
    for k in range(57, 62):
        acc = acc + x[:, k]
    for j in range(8):
        acc = acc + P[:, j]
    return acc


def sample_fine(raw_sigma, t_coarse, u, alpha_of=alpha_default, masks=None, variant=None):
    """raw_sigma [n,64] (pre-ReLU), t_coarse [64] or [n,64], u [128] or [n,128] in any order, float32 -> a dict:
        t_sorted [n,192], t_fine [n,128] (the caller's u order), valid_sorted [n,192] bool (with masks = (weights_threshold,
        ert_threshold)), the decisions per fine sample in the caller's u order (ind, below, above, live, slot = its place in t_sorted,
        valid_fine), per coarse sample (relu, passes), per ray (wsum, empty_ray, object_ray), and cdf, w, T."""
    assert raw_sigma.dtype == t_coarse.dtype == u.dtype == F32
    n, S = raw_sigma.shape
    F = u.shape[-1]
    assert S == N_SAMPLES
    t, uu = _rows(t_coarse, n).contiguous(), _rows(u, n).contiguous()
    w, T, alpha, om, q = weights(raw_sigma, t, alpha_of, variant)
    wp = w[:, 1:S - 1] + f32(EPS_W)
    wsum = torch_sum62(wp, variant)
    pdf = div_rn(wp, wsum[:, None].expand(n, S - 2))
    cdf = torch.zeros(n, S - 1, dtype=F32)
    for m in range(1, S - 1):
        cdf[:, m] = cdf[:, m - 1] + pdf[:, m - 1]
    ind = torch.searchsorted(cdf, uu, right=variant != "left")
    top = S - 2 if variant == "clamp62" else S - 3
    below, above = torch.clamp(ind - 1, 0, top), torch.clamp(ind, max=top)
    bins = 0.5 * (t[:, 1:] + t[:, :-1])
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    draw = ca - cb
    live = ~(draw < f32(EPS_W))
    denom = torch.where(live, draw, torch.ones_like(draw))
    fine = bb + div_rn(uu - cb, denom) * (ba - bb)
    assert fine.dtype == F32
    # the kernel walks the u ascending, keeps the fine depths ascending by a stable insertion, then merges with the coarse first on ties:
    # one stable sort of (coarse | fine in ascending-u order)
    by_u = torch.sort(uu, dim=1, stable=True).indices
    fine_asc = torch.gather(fine, 1, by_u)
    cat = torch.cat([fine_asc, t], dim=1) if variant == "fine_first" else torch.cat([t, fine_asc], dim=1)
    order = torch.sort(cat, dim=1, stable=True)
    place = torch.empty_like(order.indices)
    place.scatter_(1, order.indices, torch.arange(S + F)[None, :].expand(n, S + F).contiguous())
    slot_asc = place[:, :F] if variant == "fine_first" else place[:, S:]
    slot = torch.empty_like(slot_asc)
    slot.scatter_(1, by_u, slot_asc)
    out = {"t_sorted": order.values, "t_fine": fine, "ind": ind, "below": below, "above": above, "live": live, "slot": slot,
           "relu": raw_sigma > 0, "passes": (om >= f32(1e-10)) & (om <= 1.0), "wsum": wsum, "cdf": cdf, "w": w, "T": T, "om": om,
           "inversions": int((fine_asc[:, 1:] < fine_asc[:, :-1]).sum()),
           "ties": int((fine[:, :, None] == t[:, None, :]).sum())}
    sig = torch.clamp_min(raw_sigma, 0.0)
    dsum, dmax = torch.zeros(n, dtype=F32), torch.zeros(n, dtype=F32)
    for k in range(S):
        dsum = dsum + sig[:, k]
        dmax = torch.maximum(dmax, sig[:, k])
    out["dsum"], out["dmax"] = dsum, dmax
    out["empty_ray"], out["object_ray"] = dsum < f32(1e-3), dmax > f32(0.5)
    if masks is not None:
        wthr, ethr = f32(masks[0]), f32(masks[1])
        empty_bins = w[:, 1:S - 1] < wthr
        ert = torch.cummax((T[:, 1:S - 1] < ethr).to(torch.uint8), dim=1).values.bool()
        low = torch.clamp(below, max=S - 3)            # (the wrong clamp62 variant may point one past the 62 inner bins)
        high = torch.clamp(above, max=S - 3)
        be, ae, er = torch.gather(empty_bins, 1, low), torch.gather(empty_bins, 1, high), torch.gather(ert, 1, low)
        ess = torch.where(out["object_ray"][:, None], be & ae, be | ae)
        valid_fine = ~(ess | er | out["empty_ray"][:, None])
        vcat = torch.cat([torch.ones(n, S, dtype=torch.bool), torch.gather(valid_fine, 1, by_u)], dim=1)
        if variant == "fine_first":
            vcat = torch.cat([vcat[:, S:], vcat[:, :S]], dim=1)
        out["valid_fine"], out["valid_sorted"] = valid_fine, torch.gather(vcat, 1, order.indices)
    return out


def composite(raw, t, white, alpha_of=alpha_default, sigmoid=sigmoid_default, variant=None):
    """raw [n,S,4], t [S] or [n,S], float32 -> (rgb [n,3], depth [n], weights [n,S]) in CompositeAcc's order: per sample
    c = fadd(c, fmul(w, sigmoid(raw_c))), d = fadd(d, fmul(w, t)), acc = fadd(acc, w); with a white background c = fadd(c, fsub(1, acc))."""
    assert raw.dtype == t.dtype == F32
    n, S = raw.shape[0], raw.shape[1]
    t = _rows(t, n).contiguous()
    w = weights(raw[:, :, 3].contiguous(), t, alpha_of, variant)[0]
    col = sigmoid(raw[:, :, :3].contiguous())
    assert col.dtype == F32
    rgb, depth, acc = torch.zeros(n, 3, dtype=F32), torch.zeros(n, dtype=F32), torch.zeros(n, dtype=F32)
    for k in range(S):
        rgb = rgb + w[:, k, None] * col[:, k]
        depth = depth + w[:, k] * t[:, k]
        acc = acc + w[:, k]
    if white:
        rgb = rgb + (1.0 - acc)[:, None]
    return rgb, depth, w


# ---- the adjoints' twins ---------------------------------------------------------------------------------------------------------------
def _smooth_weights(sigma_leaf, t, relu, passes, dtype, variant=None):
    """w [n,S] in `dtype`, differentiable in sigma_leaf and t, with the relu mask, the clamp-pass mask and the last delta as constants."""
    n, S = sigma_leaf.shape
    sigma = torch.where(relu, sigma_leaf, torch.zeros_like(sigma_leaf))
    last = torch.full((n, 1), 1e10, dtype=dtype)
    if variant == "last_delta_from_t" and S > 1:
        last = t[:, -1:] - t[:, -2:-1]
    delta = torch.cat([t[:, 1:] - t[:, :-1], last], dim=1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    om = 1.0 - alpha
    q = torch.where(passes, om, torch.clamp(om, min=1e-10, max=1.0).detach())
    Ts, T = [], torch.ones(n, dtype=dtype)
    for k in range(S):
        Ts.append(T)
        T = T * q[:, k]
    return torch.stack(Ts, dim=1) * alpha


def pass_mask(om, variant=None):
    if variant == "pass_strict":
        return (om > f32(1e-10)) & (om < 1.0)
    return (om >= f32(1e-10)) & (om <= 1.0)


def composite_twin(raw, t, white, g_rgb, g_depth, dtype, alpha_of=alpha_default, variant=None):
    """The adjoint of `composite` for the cotangents g_rgb [n,3], g_depth [n] (None: zero) -> (g_raw [n,S,4], g_t [n,S]) in `dtype`.
    The relu mask and the clamp-pass mask come from the fp32 restatement (with `alpha_of`), the last delta is the constant 1e10."""
    n, S = raw.shape[0], raw.shape[1]
    t32 = _rows(t, n).contiguous()
    om = weights(raw[:, :, 3].contiguous(), t32, alpha_of)[3]
    x = raw.to(dtype).clone().requires_grad_(True)
    tt = t32.to(dtype).clone().requires_grad_(True)
    w = _smooth_weights(x[:, :, 3], tt, raw[:, :, 3] > 0, pass_mask(om, variant), dtype, variant)
    rgb = (w[:, :, None] * torch.sigmoid(x[:, :, :3])).sum(1)
    if white:
        rgb = rgb + (1.0 - w.sum(1))[:, None]
    loss = (rgb * g_rgb.to(dtype)).sum()
    if g_depth is not None:
        loss = loss + ((w * tt).sum(1) * g_depth.to(dtype)).sum()
    g_raw, g_t = torch.autograd.grad(loss, [x, tt], allow_unused=True)
    return g_raw, (torch.zeros_like(tt) if g_t is None else g_t)


def sample_twin(raw_sigma, t_coarse, u, g_t_sorted, dtype, decisions, variant=None):
    """The adjoint of `sample_fine` for the cotangent g_t_sorted [n,192] -> g_raw_coarse[..., 3] [n,64] in `dtype`; `decisions` is
    sample_fine's dict on the same inputs (bins, live, slot, relu and clamp-pass masks).  The coarse depths and u are constants."""
    n, S = raw_sigma.shape
    t, uu = _rows(t_coarse, n).to(dtype), _rows(u, n).to(dtype)
    d = decisions
    x = raw_sigma.to(dtype).clone().requires_grad_(True)
    w = _smooth_weights(x, t, d["relu"], pass_mask(d["om"], variant), dtype, variant)
    wp = w[:, 1:S - 1] + float(f32(EPS_W))                     # the forward's constant, the float
    pdf = wp / wp.sum(1, keepdim=True)
    run, cols = torch.zeros(n, dtype=dtype), []
    for m in range(S - 1):                                     # a running sum in `dtype` (torch's CPU cumsum would carry fp32 in float64)
        cols.append(run)
        run = run + pdf[:, m] if m < S - 2 else run
    cdf = torch.stack(cols, dim=1)
    bins = 0.5 * (t[:, 1:] + t[:, :-1])
    cb, ca = torch.gather(cdf, 1, d["below"]), torch.gather(cdf, 1, d["above"])
    bb, ba = torch.gather(bins, 1, d["below"]), torch.gather(bins, 1, d["above"])
    denom = torch.where(d["live"], ca - cb, torch.ones_like(ca))
    fine = bb + (uu - cb) / denom * (ba - bb)
    loss = (fine * torch.gather(g_t_sorted.to(dtype), 1, d["slot"])).sum()
    return torch.autograd.grad(loss, [x])[0]


def rule(hip, f64, cpu32):
    """The project's rule on rays divided by their own max|f64|: -> (measured, allowed, zero_rows_ok) with
    measured = max|hip - f64|, allowed = 3 max|cpu_fp32 - f64| + 2 u max|f64| over the normalised rays; a ray whose float64
    gradient is zero must be exactly zero in `hip`."""
    n = f64.shape[0]
    f64, hip, cpu32 = f64.double().reshape(n, -1), hip.double().reshape(n, -1), cpu32.double().reshape(n, -1)
    scale = f64.abs().amax(dim=1)
    zero = scale == 0
    zero_ok = bool((hip[zero] == 0).all())
    if bool(zero.all()):
        return 0.0, 0.0, zero_ok
    s = scale[~zero, None]
    d_hip = float(((hip[~zero] - f64[~zero]) / s).abs().max())
    d_cpu = float(((cpu32[~zero] - f64[~zero]) / s).abs().max())
    return d_hip, 3 * d_cpu + 2 * U * 1.0, zero_ok


# ---- edge rays -------------------------------------------------------------------------------------------------------------------------
OPAQUE = 1e4                       # sigma * delta >= 1e4 * (4 / 192) = 208: exp underflows, alpha = 1, 1 - alpha = 0 < 1e-10
N_EDGE = 67                        # two 64-ray workgroups of the forward (3 rays in the second); 16 four-ray blocks of the adjoint + 3


def _seq_sum(x):
    acc = f32(0.0)
    for v in x:
        acc = acc + v
    return acc


def _row_with_sum(gen, target):
    """64 positive densities whose sequential fp32 sum is exactly `target` (float32)."""
    row = torch.rand(64, generator=gen) * float(target) / 40.0
    for _ in range(64):
        s63 = _seq_sum(row[:63])
        row[63] = target - s63
        if _seq_sum(row) == target and row[63] > 0:
            return row
        row[62] = torch.nextafter(row[62], f32(0.0))
    raise AssertionError("no row with that sum")


def sampler_rays(seed=0):
    """-> (raw_coarse [67,64,4] with NaN in the rgb columns, {family: [row ids]})."""
    gen = torch.Generator().manual_seed(1000 + seed)
    semi = lambda: torch.exp(torch.randn(64, generator=gen)) * 0.8          # noqa: E731
    rows, fam = [], {}

    def add(name, row):
        fam.setdefault(name, []).append(len(rows))
        rows.append(row.to(F32))

    dead = -torch.rand(64, generator=gen)
    dead[::3], dead[1::3] = -0.0, 0.0
    add("dead", dead)
    add("dead", torch.full((64,), -0.0))
    for idx in (1, 31, 62):
        for name, rest in (("one_opaque_alone", torch.full((64,), -1.0)), ("one_opaque", semi())):
            row = rest.clone()
            row[idx] = OPAQUE
            add(name, row)
    for rest in (torch.full((64,), -1.0), semi() * 0.1):
        row = rest.clone()
        row[0], row[63] = OPAQUE, OPAQUE
        add("opaque_ends", row)
    for start in (0, 10, 58):
        row = semi() * 0.2
        row[start:start + 5] = OPAQUE
        add("five_opaque_first" if start == 0 else "five_opaque", row)          # (behind five opaque samples fp32 sees nothing at all)
    add("tiny", torch.full((64,), 1e-30))
    milli = f32(1e-3)
    for target in (torch.nextafter(milli, f32(0.0)), milli, torch.nextafter(milli, f32(1.0))):
        add("sum_1e-3", _row_with_sum(gen, target))
    for top in (f32(0.5), torch.nextafter(f32(0.5), f32(1.0))):
        for _ in range(2):
            row = torch.rand(64, generator=gen) * 0.49
            row[torch.rand(64, generator=gen) < 0.3] = -1.0
            row[int(torch.randint(1, 63, (1,), generator=gen))] = top
            add("max_0.5", row)
    for _ in range(20):
        row = torch.exp(2.0 * torch.randn(64, generator=gen))
        row[torch.rand(64, generator=gen) < 0.7] *= -1.0
        add("random", row)
    with np.load(os.path.join(GOLDEN, "sampling.npz")) as z:
        scene = torch.from_numpy(z["raw_coarse"][:N_EDGE - len(rows), :, 3])
    for row in scene:
        add("scene", row.clone())
    assert len(rows) == N_EDGE
    raw = torch.full((N_EDGE, 64, 4), float("nan"))
    raw[:, :, 3] = torch.stack(rows)
    return raw.contiguous(), fam


def stratified(t_table, jitter):
    """nerf_stratified_samples' formula: lower + (upper - lower) * jitter between the mid points of the table."""
    mids = 0.5 * (t_table[1:] + t_table[:-1])
    lower, upper = torch.cat([t_table[:1], mids]), torch.cat([mids, t_table[-1:]])
    return lower + (upper - lower) * jitter


def tie_us(t_table, bins_at=(5, 20, 40)):
    """u values whose fine depth IS a coarse depth, bit for bit, on a ray without weight (w = 0 everywhere, whatever exp is: the rays
    of sigma <= 0 and of sigma = 1e-30, whose cdf is the uniform one): for bin b the float u around the solution of
    fine(u) = t[b + 1], found by trying its neighbours."""
    found = []
    sigma = torch.full((1, 64), -1.0)
    cdf = sample_fine(sigma, t_table, torch.zeros(128))["cdf"][0]
    bins = 0.5 * (t_table[1:] + t_table[:-1])
    for b in bins_at:
        u0 = cdf[b] + (t_table[b + 1] - bins[b]) / (bins[b + 1] - bins[b]) * (cdf[b + 1] - cdf[b])
        cand = (u0.view(torch.int32) + torch.arange(-512, 512, dtype=torch.int32)).view(F32)
        hit = sample_fine(sigma, t_table, cand)["t_fine"][0] == t_table[b + 1]
        assert bool(hit.any()), b
        found.append(cand[hit][0])
    return torch.stack(found)


def sampler_tables(seed=0):
    """-> {"t": {0: [64], 64: [67,64]}, "u": {0: [128] linspace, "tie": [128] ascending, 128: [67,128] unsorted}}, keyed by the ray
    stride; "tie" is a second shared table (stride 0) that holds tie_us of the linspace depths, as do the per-ray u rows of the
    rays without weight."""
    gen = torch.Generator().manual_seed(2000 + seed)
    t_lin, u_lin = torch.linspace(2.0, 6.0, 64), torch.linspace(0.0, 1.0, 128)
    jitter = torch.rand(N_EDGE, 64, generator=gen)
    jitter[0], jitter[1] = 0.0, 1.0 - U
    u = torch.rand(N_EDGE, 128, generator=gen)
    u[:, 5], u[:, 77], u[:, 100] = 0.0, 1.0 - U, 1.0
    u[:, 60:64] = u[:, 20:24]                                   # duplicates
    u[2] = u_lin.flip(0)                                        # descending
    u[3] = 0.5
    ties = tie_us(t_lin)
    fam = sampler_rays(seed)[1]
    for r in fam["dead"] + fam["tiny"]:
        u[r, 30:30 + ties.shape[0]] = ties
    u_tie = u_lin.clone()
    u_tie[40:40 + ties.shape[0]] = ties
    u_tie = torch.sort(u_tie).values
    return {"t": {0: t_lin, 64: stratified(t_lin, jitter).contiguous()}, "u": {0: u_lin, "tie": u_tie.contiguous(), 128: u.contiguous()}}


def u_stride(us):
    return 0 if us == "tie" else us


COMPOSITE_S = (1, 2, 15, 16, 17, 63, 64, 65, 128, 191, 192)
COMPOSITE_N = (1, 3, 5, 67)
COMPOSITE_FAMILIES = ("semi", "dead", "one_opaque", "several_opaque", "repeated_depths", "rgb_extremes")


def composite_rays(S, seed=0):
    """-> (raw [67,S,4], t [67,S] ascending, family id per ray [67]); ray i belongs to family i % 6."""
    gen = torch.Generator().manual_seed(3000 + 7 * S + seed)
    n = N_EDGE
    raw = torch.randn(n, S, 4, generator=gen)
    raw[:, :, 3] = torch.exp(torch.randn(n, S, generator=gen)) * (0.03 * S)          # sigma * delta of order 0.1
    raw[:, :, 3][torch.rand(n, S, generator=gen) < 0.3] *= -1.0
    t = torch.sort(2.0 + 4.0 * torch.rand(n, S, generator=gen), dim=1).values
    family = torch.arange(n) % len(COMPOSITE_FAMILIES)
    for i in range(n):
        f = COMPOSITE_FAMILIES[int(family[i])]
        at = int(torch.randint(0, S, (1,), generator=gen))
        if f == "dead":
            raw[i, :, 3] = -torch.rand(S, generator=gen)
            raw[i, ::2, 3] = -0.0
            raw[i, 1::4, 3] = 0.0
        elif f == "one_opaque":
            raw[i, at, 3] = OPAQUE * 192
        elif f == "several_opaque":
            lo = min(at, max(S - 6, 0))                       # one sample behind the five sees T = 0
            raw[i, lo:lo + 5, 3] = OPAQUE * 192
            raw[i, S - 1, 3] = 1.0
        elif f == "repeated_depths":
            t[i, 1::2] = t[i, 0:S - 1:2][:t[i, 1::2].shape[0]]
            raw[i, :, 3] = raw[i, :, 3].abs()
        elif f == "rgb_extremes":
            vals = torch.tensor([100.0, -100.0, 0.0, -0.0])
            raw[i, :, :3] = vals[torch.randint(0, 4, (S, 3), generator=gen)]
    return raw.contiguous(), t.contiguous(), family


def subset(n):
    """The rays of the 67 a call with n rays gets: spread over the set, so that small counts still meet several families."""
    return torch.arange(n) * (N_EDGE // n) if n < N_EDGE else torch.arange(N_EDGE)


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def read_record():
    if not os.path.exists(RAY_SIDE_JSON):
        return {}
    with open(RAY_SIDE_JSON) as f:
        return json.load(f)


def record(key, stats):
    """Keep measured figures: merged into profiles/ray_side.json under `key` (hashfield_sampling_reference.record's convention, its
    copy directory included)."""
    rec = read_record()
    rec[key] = stats
    os.makedirs(os.path.dirname(RAY_SIDE_JSON), exist_ok=True)
    with open(RAY_SIDE_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(RAY_SIDE_JSON, os.path.join(out, os.path.basename(RAY_SIDE_JSON)))
