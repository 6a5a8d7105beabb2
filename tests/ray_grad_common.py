"""CPU side of the ray-gradient tests (tests/test_gpu_ray_grad.py): d loss / d (rays_o, rays_d) of the reference's render with the
rays as autograd leaves, evaluated

  * in fp32 by the reference's own arithmetic (oracle.render; stochastic_common.render with recorded draws), and
  * entirely in float64 on the same fp32 inputs, weights and depth tables (in the style of train_steps_common.staged_step_fp64):
    the truth both fp32 evaluations -- torch's on the CPU and the HIP kernels' -- are judged against,

plus the per-ray bins of the inverse-CDF sampler, so that rays on which fp32 and float64 pick other bins (the sampler's
discontinuity) can be told apart from adjoint arithmetic.  The loss is the one the tests use for both outputs:
mse(rgb, target) + 0.1 depth.mean().
"""
import torch

import nerf_oracle as orc
import stochastic_common as SC


def loss_of(rgb, depth, target):
    return torch.nn.functional.mse_loss(rgb, target) + 0.1 * depth.mean()


def sampler_bins(sigma_c, t_c, u, eps=1e-5):
    """(below, above) [n,128] of the inverse-CDF sampler on ReLU'd coarse densities, in their dtype."""
    with torch.no_grad():
        _, w = orc.transmittance_weights(sigma_c, t_c)
        w = w[:, 1:-1] + eps
        cdf = torch.cumsum(w / torch.sum(w, -1, keepdim=True), -1)
        cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
        inds = torch.searchsorted(cdf, u.to(cdf.dtype).contiguous(), right=True)
        n_s = t_c.shape[1]
        return torch.clamp(inds - 1, 0, n_s - 3), torch.clamp(inds, 0, n_s - 3)


def _u_table(u, n):
    return orc.fine_u().expand(n, orc.N_IMPORTANCE) if u is None else u


def ray_grads_fp32(sd, o, d, target, jitter=None, u=None):
    """The reference's fp32 render (deterministic: oracle.render; with draws: stochastic_common.render) under torch autograd
    -> (g_o [n,3], g_d [n,3], bins)."""
    o = o.detach().clone().requires_grad_(True)
    d = d.detach().clone().requires_grad_(True)
    n = o.shape[0]
    if jitter is None and u is None:
        rgb, dep, parts = orc.render(sd, o[None], d[None], return_parts=True)
    else:
        rgb, dep, parts = SC.render(sd, o, d, jitter, u)
    loss_of(rgb, dep, target).backward()
    bins = sampler_bins(torch.relu(parts["raw_coarse"][..., 3].detach()), parts["t_coarse"], _u_table(u, n))
    return o.grad.detach(), d.grad.detach(), bins


def ray_grads_fp64(sd, o, d, target, jitter=None, u=None):
    """The same loss and backward pass entirely in float64 (encoding, both MLPs, sampler, compositing) on the fp32 inputs,
    weights and depth tables -> (g_o, g_d, bins), float64."""
    sd64 = {k: sd[k].detach().double() for k in orc.state_dict_keys()}
    o = o.detach().double().requires_grad_(True)
    d = d.detach().double().requires_grad_(True)
    n = o.shape[0]
    t_c = SC.stratified_t(jitter, n).double()
    u64 = _u_table(u, n).double().contiguous()
    vd = d / torch.norm(d, dim=-1, keepdim=True)

    def mlp(prefix, pts):
        s = pts.shape[1]
        flat = pts.reshape(-1, 3)
        dflat = vd[:, None].expand(n, s, 3).reshape(-1, 3)
        emb = torch.cat([orc.freq_encode(flat, orc.XYZ_FREQS), orc.freq_encode(dflat, orc.DIR_FREQS)], -1)
        return orc.nerf_mlp(sd64, prefix, emb).reshape(n, s, 4)

    pts_c = orc.points_on_rays(o, d, t_c)
    raw_c = mlp("model", pts_c)
    sigma_c = torch.relu(raw_c[..., 3])
    _, w = orc.transmittance_weights(sigma_c, t_c)
    w = w[:, 1:-1] + 1e-5
    cdf = torch.cumsum(w / torch.sum(w, -1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    inds = torch.searchsorted(cdf.detach(), u64, right=True)
    below, above = torch.clamp(inds - 1, 0, 61), torch.clamp(inds, 0, 61)
    bins = 0.5 * (t_c[:, 1:] + t_c[:, :-1])
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = ca - cb
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t_f = bb + (u64 - cb) / denom * (ba - bb)
    pts_f = orc.points_on_rays(o, d, t_f)
    depth, order = torch.sort(torch.cat([t_c, t_f], 1), dim=-1)
    pts = torch.gather(torch.cat([pts_c, pts_f], 1), 1, order[..., None].expand(-1, -1, 3))
    raw_f = mlp("model_fine", pts)
    rgb, dep = orc.composite(raw_f, depth, True)
    loss_of(rgb, dep, target.double()).backward()
    return o.grad.detach(), d.grad.detach(), (below, above)


def per_ray_errors(g64, *gs):
    """Per-ray error of each (g_o, g_d) in `gs` against the float64 one: max over the 6 components of |g - g64|, divided by the
    ray's own scale (its largest float64 component, floored at 1e-3 of the batch's largest: rays that see nothing have ~0)."""
    t = torch.cat([g64[0], g64[1]], 1).double()
    scale = t.abs().amax(1).clamp_min(1e-3 * t.abs().max().item())
    return [(torch.cat([g[0], g[1]], 1).double() - t).abs().amax(1) / scale for g in gs]
