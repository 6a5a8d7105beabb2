"""CPU restatement of the reference's stochastic (task == "train") sampling, from the oracle's pieces.

The reference draws the coarse jitter (volume_renderer.py:48-60) and the inverse-CDF u (:143-147) with torch.rand; here both
are arguments, so recorded draws (tests/golden/stochastic_*.npz, tools/gen_stochastic_golden.py) replay exactly.  Pinned
bit for bit against the reference by tests/test_stochastic_host.py; the GPU tests compare against it.
"""
import torch

import nerf_oracle as orc


def stratified_t(jitter, n=None):
    """jitter [n,64] (or None: the deterministic table) -> t_coarse [n,64], the reference's expression."""
    t = orc.stratified_t()
    if jitter is None:
        return t.unsqueeze(0).expand(n, orc.N_SAMPLES).clone()
    mids = 0.5 * (t[1:] + t[:-1])
    lower = torch.cat([t[:1], mids], 0).unsqueeze(0).expand_as(jitter)
    upper = torch.cat([mids, t[-1:]], 0).unsqueeze(0).expand_as(jitter)
    return lower + (upper - lower) * jitter


def inverse_cdf(sigma_c, t_c, u, eps=1e-5):
    """oracle.fine_sample with the u of every ray given: sigma_c (ReLU'd), t_c [n,64], u [n,128] -> t_fine [n,128]."""
    n_s = t_c.shape[1]
    _, w = orc.transmittance_weights(sigma_c, t_c)
    w = w[:, 1:-1] + eps
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, 0, n_s - 3)
    above = torch.clamp(inds, 0, n_s - 3)
    bins = 0.5 * (t_c[:, 1:] + t_c[:, :-1])
    cdf_b, cdf_a = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bin_b, bin_a = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = cdf_a - cdf_b
    denom = torch.where(denom < eps, torch.ones_like(denom), denom)
    return bin_b + (u - cdf_b) / denom * (bin_a - bin_b)


def render(sd, rays_o, rays_d, jitter, u, raw_coarse=None, t_sorted=None, chunk=orc.MLP_CHUNK, mlp_dtype=torch.float32):
    """The reference's no-grad render in training sampling mode -> (rgb, depth, parts).  u None: the deterministic linspace.
    `raw_coarse` / `t_sorted` given: used instead of the recomputed ones (attribution of a deviation to moved samples)."""
    n = rays_o.shape[0]
    t_c = stratified_t(jitter, n)
    vd = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    if raw_coarse is None:
        raw_coarse = orc.network_forward(sd, orc.points_on_rays(rays_o, rays_d, t_c), vd, "", chunk, mlp_dtype)
    if u is None:
        u = orc.fine_u().expand(n, orc.N_IMPORTANCE)
    if t_sorted is None:
        t_f = inverse_cdf(torch.relu(raw_coarse[..., 3]), t_c, u)
        t_sorted, _ = torch.sort(torch.cat([t_c, t_f], 1), dim=-1)
    pts = orc.points_on_rays(rays_o, rays_d, t_sorted)
    raw = torch.cat([orc.network_forward(sd, pts[:, j:j + orc.SAMPLE_BLOCK], vd, "fine", chunk, mlp_dtype)
                     for j in range(0, pts.shape[1], orc.SAMPLE_BLOCK)], 1)
    rgb, dep = orc.composite(raw, t_sorted)
    return rgb, dep, dict(t_coarse=t_c, raw_coarse=raw_coarse, t_sorted=t_sorted)


def adam_losses(sd0, g, chunk=orc.MLP_CHUNK, mlp_dtype=torch.float32):
    """The reference's K-step loop (MSE, backward, clip 40, Adam 5e-4) on the restatement with the recorded draws of
    stochastic_train_steps.npz, MLP evaluated `chunk` points at a time (in `mlp_dtype`) -> per-step losses.  fp32 vs a float64
    MLP bounds how far the reference's own fp32 rounding moves its trajectory (tests/test_train_noise_floor.py)."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 5e-4, "weight_decay": 0.0, "eps": 1e-8} for p in params.values()],
                           5e-4, weight_decay=0.0, eps=1e-8)
    losses = []
    for s in range(int(g["K"])):
        rgb, _, _ = render(params, g["rays_o"], g["rays_d"], g["jitter"][s], g["u"][s], chunk=chunk, mlp_dtype=mlp_dtype)
        loss = torch.nn.functional.mse_loss(rgb, g["target"])
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(list(params.values()), 40)
        opt.step()
        losses.append(loss.item())
    return losses


def fixture_runs(g):
    """(tag, state-dict name, jitter or None, u) of the runs in stochastic_render.npz."""
    return [(tag, fam, g.get(f"{tag}_jitter"), g[f"{tag}_u"])
            for tag, fam in (("trained", "trained"), ("sharp", "sharp"), ("trained_u", "trained"))]


def family_sd(oracle, base_sd, fam):
    import os
    from conftest import GOLDEN
    if fam == "trained":
        ck = torch.load(os.path.join(GOLDEN, "trained_ckpt.pth"), weights_only=True)["net"]
        return {k: ck[k] for k in oracle.state_dict_keys()}
    return oracle.weight_family(base_sd, fam)
