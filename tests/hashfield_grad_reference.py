"""Restatement of the hash field's spatial adjoint (include/nerf_mi355x_field.h), in torch on the CPU: the
yardstick of tests/test_hashfield_grad_cpu.py and tests/test_gpu_hashfield_grad.py.  A helper, not a test; written from the formulas
of the header, not from any kernel; it imports hashfield_reference / hashgrid_reference / fused_mlp_reference and nothing of the package.

    glue, fp32 fixed order   seed, points_backward, ray_sums, sh_gradient, sh4_backward: with float32 every operation is one separately
                             rounded torch op in the header's order (the per-ray sums in the documented lane / fold order), so the
                             kernels match them bit for bit; with float64 the same formulas are the truth
    by hand, float64         density_gradient_by_hand: the launch chain of HashField.density_gradient from the pieces
    differentiable field     density_gradient, geometry, render_rays: autograd through the restated field in the parameters' dtype
                             (float64: the truth, float32: cpu_fp32), the positions and view directions carrying their derivative
"""
import os

import numpy as np
import torch

import fused_mlp_reference as F
import hashfield_reference as R
import hashgrid_reference as H

PARITY_JSON = os.path.join(R.REPO, "profiles", "hashfield_grad_parity.json")
GEO = R.GEO
C1, C2, C3, C4, C5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.54627421529603959, 0.59004358992664352
C6, C7, C8, C9 = 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769


def parity_record(key, stats):
    """R.parity_record's pattern on profiles/hashfield_grad_parity.json."""
    saved = R.PARITY_JSON
    R.PARITY_JSON = PARITY_JSON
    try:
        R.parity_record(key, stats)
    finally:
        R.PARITY_JSON = saved


# ---- glue ----------------------------------------------------------------------------------------------------------------------------
def seed(sigma_rows, positive_only):
    """seed [M,16]: column 0 is 0 where positive_only and not sigma > 0, else 1; the other columns 0."""
    out = torch.zeros(sigma_rows.shape[0], GEO, dtype=sigma_rows.dtype)
    out[:, 0] = torch.where(~(sigma_rows > 0), 0.0, 1.0) if positive_only else 1.0
    return out


def world_points(o, d, t, S, index, n_rows):
    """The forward's p of every row, float32 with its two roundings, and the row's depth (0 in point mode)."""
    ids = R.ids_of(index, n_rows)
    ray, s = ids // S, ids % S
    if d is None:
        assert S == 1
        return o[ray], torch.zeros(n_rows, dtype=torch.float32)
    p = o[ray] + d[ray] * t[s][:, None]
    assert p.dtype == torch.float32
    return p, t[s]


def points_backward(o, d, t, S, index, n_rows, frame, g_x):
    """g_p [n_rows,3] (compact) in g_x's dtype: div_rn(g_x, extent) where lo <= p <= hi, +0 elsewhere."""
    lo, hi, extent = frame
    p, _ = world_points(o, d, t, S, index, n_rows)
    inside = (p >= lo[None]) & (p <= hi[None])
    if g_x.dtype == torch.float32:
        q = R.div_rn(g_x, torch.full_like(g_x, extent))
    else:
        q = g_x / extent
    return torch.where(inside, q, torch.zeros_like(q))


def by_id(g_p, index, n_rows, n_points, fill):
    out = torch.full((n_points, 3), fill, dtype=g_p.dtype)
    out[R.ids_of(index, n_rows)] = g_p[:n_rows]
    return out


def runs(index, n_rows, n_rays, S):
    """[(a, b)] per ray: the rows whose id lies in [r S, r S + S), by binary search over the ascending ids."""
    ids = R.ids_of(index, n_rows).numpy()
    first = np.arange(n_rays, dtype=np.int64) * S
    return list(zip(np.searchsorted(ids, first, side="left").tolist(), np.searchsorted(ids, first + S, side="left").tolist()))


def wave_sum(terms):
    """The documented order of a per-ray sum over terms [k, ...]: lane l adds rows l, l + 64, ... from +0, then the 64 partial sums
    are folded v[l] += v[l + h], h = 32 .. 1.  Every add is one torch op in the terms' dtype."""
    k = terms.shape[0]
    pad = (-k) % 64
    if pad or k == 0:
        terms = torch.cat([terms, torch.zeros((pad if k else 64,) + tuple(terms.shape[1:]), dtype=terms.dtype)], 0)
    terms = terms.reshape(-1, 64, *terms.shape[1:])
    v = torch.zeros_like(terms[0])
    for block in terms:
        v = v + block                                # (a lane past the run adds +0: the value does not move)
    h = 32
    while h:
        v = v[:h] + v[h:2 * h]
        h //= 2
    return v[0]


def ray_sums(o, d, t, S, index, n_rows, frame, g_x, g_view=None):
    """(g_rays_o, g_rays_d) [n,3] in g_x's dtype: sum g_p and sum fmul(t, g_p) over each ray's run, then + g_view."""
    n = o.shape[0]
    g_p = points_backward(o, d, t, S, index, n_rows, frame, g_x)
    _, tt = world_points(o, d, t, S, index, n_rows)
    tg = tt.to(g_p.dtype)[:, None] * g_p
    g_o = torch.stack([wave_sum(g_p[a:b]) for a, b in runs(index, n_rows, n, S)])
    g_d = torch.stack([wave_sum(tg[a:b]) for a, b in runs(index, n_rows, n, S)])
    return g_o, (g_d if g_view is None else g_d + g_view)


def sh_gradient(g_cin, index, n_rows, n_rays, S):
    return torch.stack([wave_sum(g_cin[a:b, GEO:]) for a, b in runs(index, n_rows, n_rays, S)])


def sh4_backward(d, g_sh):
    """d [n,3] float32, g_sh [n,16] -> g_rays_d_view [n,3] in g_sh's dtype: the header's polynomial adjoint, term by term in its
    order and parentheses, then the normalisation's."""
    assert d.dtype == torch.float32
    dtype = g_sh.dtype
    d = d.to(dtype)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    s = (x * x + y * y) + z * z
    r = R.sqrt_rn(s)
    x, y, z = R.div_rn(x, r), R.div_rn(y, r), R.div_rn(z, r)
    g = [g_sh[:, k] for k in range(16)]
    q = 1.0 - ((5.0 * z) * z)
    m = (y * y) - (x * x)
    c5m3 = (C5 * m) * 3.0
    c5xy = (C5 * x) * y
    c7q = C7 * q
    gx = g[3] * -C1
    for term in (g[4] * (C2 * y), g[7] * (-C2 * z), g[8] * ((C4 * x) * 2.0), g[9] * (c5xy * -6.0), g[10] * ((C6 * y) * z), g[13] * c7q,
                 g[14] * (((C9 * x) * z) * 2.0), g[15] * c5m3):
        gx = gx + term
    gy = g[1] * -C1
    for term in (g[4] * (C2 * x), g[5] * (-C2 * z), g[8] * ((C4 * y) * -2.0), g[9] * c5m3, g[10] * ((C6 * x) * z), g[11] * c7q,
                 g[14] * (((C9 * y) * z) * -2.0), g[15] * (c5xy * 6.0)):
        gy = gy + term
    gz = g[2] * C1
    for term in (g[5] * (-C2 * y), g[6] * ((C3 * z) * 2.0), g[7] * (-C2 * x), g[10] * ((C6 * x) * y), g[11] * (((C7 * y) * z) * -10.0),
                 g[12] * (C8 * (((15.0 * z) * z) - 3.0)), g[13] * (((C7 * x) * z) * -10.0), g[14] * (C9 * ((x * x) - (y * y)))):
        gz = gz + term
    w = (x * gx + y * gy) + z * gz
    return torch.stack([R.div_rn(gx - x * w, r), R.div_rn(gy - y * w, r), R.div_rn(gz - z * w, r)], dim=1)


def sh4_differentiable(d):
    """The basis of d / |d| as plain differentiable torch in d's dtype (any order): what autograd differentiates."""
    u = d / d.norm(dim=1, keepdim=True)
    return R._sh4_unit(u[:, 0], u[:, 1], u[:, 2])


# ---- the field with its positions carrying a derivative ------------------------------------------------------------------------------
def hash_forward_x(x32, xd, emb, offsets, scales):
    """R.hash_forward with the fraction extended linearly in xd around the float32 position: f = f32 + (xd - x32) * scale.  At
    xd = x32 the values are R.hash_forward's; the derivative with respect to xd is the encoding's, and inside the cell the function
    of xd is the exact multilinear one (what central differences probe)."""
    B, D = x32.shape
    dtype = emb.dtype
    C, L = emb.shape[1], len(offsets) - 1
    outs = []
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        g, f32 = H.cells(x32, scales[l])
        f = f32.to(dtype) + (xd - x32.to(dtype)) * float(np.float32(scales[l]))
        omf = 1 - f
        acc = torch.zeros(B, C, dtype=dtype)
        for idx in range(1 << D):
            rows = H.corner_rows(g, idx, n, scales[l]) + int(offsets[l])
            acc = acc + H.corner_weight(f, idx, omf)[:, None] * emb[rows]
        outs.append(acc)
    return torch.cat(outs, dim=1)


def sigma_of(params, x32, xd, offsets, scales):
    """(geo [M,16], pres) at the normalised positions, differentiable with respect to xd."""
    return R.mlp(hash_forward_x(x32, xd, params["emb"], offsets, scales), params["sw"], params["sb"])


def density_gradient(params, xyz, frame, offsets, scales, positive_only=False, want_pres=False):
    """(sigma [n], grad [n,3]) at world points xyz (float32) in the parameters' dtype, the gradient by autograd through the field and
    the normalisation's adjoint (zero on a clamped axis)."""
    dtype = params["emb"].dtype
    n = xyz.shape[0]
    x32 = R.points(xyz, None, None, 1, None, n, frame)
    xd = x32.to(dtype).requires_grad_(True)
    geo, pres = sigma_of(params, x32, xd, offsets, scales)
    sigma = geo[:, 0]
    picked = torch.where(sigma > 0, sigma, torch.zeros_like(sigma)) if positive_only else sigma
    g_x, = torch.autograd.grad(picked.sum(), xd)
    grad = points_backward(xyz, None, None, 1, None, n, frame, g_x)
    return (sigma.detach(), grad, pres) if want_pres else (sigma.detach(), grad)


def density_gradient_by_hand(params, xyz, frame, offsets, scales, positive_only=False):
    """The launch chain of HashField.density_gradient composed from the pieces in float64: the encoding (hashgrid_reference.truth_f64),
    the network and its data gradient (fused_mlp_reference), seed, the encoding's input gradient, points_backward.  `params` fp32."""
    n = xyz.shape[0]
    x32 = R.points(xyz, None, None, 1, None, n, frame)
    enc = H.truth_f64(x32, params["emb"], offsets, scales)["out"]
    geo, _, _ = F.forward(enc, params["sw"], params["sb"], False)
    g_enc, _, _ = F.backward(enc, params["sw"], params["sb"], seed(geo[:, 0], positive_only), False)
    g_x = H.truth_f64(x32, params["emb"], offsets, scales, grad_out=g_enc)["grad_x"]
    return geo[:, 0], points_backward(xyz, None, None, 1, None, n, frame, g_x)


def _ray_rows(params, o, d, od, dd, t, frame, offsets, scales, keep):
    """The surviving rows of a scene: (index, M, x32, xd) with xd = x32 + the derivative path of (od + dd t - lo) / extent where the
    clamp passes; od, dd are o, d in the parameters' dtype (they may require grad)."""
    dtype = params["emb"].dtype
    lo, hi, extent = frame
    n, S = o.shape[0], t.shape[0]
    index = None if keep is None else torch.nonzero(keep.reshape(-1)).reshape(-1).to(torch.int32)
    M = n * S if index is None else int(index.numel())
    ids = R.ids_of(index, M)
    x32 = R.points(o, d, t, S, index, M, frame)
    p32, _ = world_points(o, d, t, S, index, M)
    inside = ((p32 >= lo[None]) & (p32 <= hi[None])).to(dtype)
    lin = inside * (od[ids // S] + dd[ids // S] * t.to(dtype)[ids % S][:, None]) / extent
    return index, M, ids, x32, x32.to(dtype) + (lin - lin.detach())


def composite_weights(sigma, t, dtype):
    """nerf_composite's weights w [n,S] from the raw densities [n,S] (R.composite's recurrence)."""
    n, S = sigma.shape
    t = t.to(torch.float32)
    delta = torch.cat([t[1:] - t[:-1], torch.tensor([1e10], dtype=torch.float32)]).to(dtype)
    T = torch.ones(n, dtype=dtype)
    ws = []
    for k in range(S):
        alpha = 1.0 - torch.exp(-torch.relu(sigma[:, k]) * delta[k])
        ws.append(T * alpha)
        T = T * torch.clamp(1.0 - alpha, min=1e-10, max=1.0)
    return torch.stack(ws, dim=1)


def geometry(params, o, d, t, frame, offsets, scales, keep=None, want_pres=False):
    """(acc [n], normal [n,3]) in the parameters' dtype: acc = sum_i w_i, normal = sum_i w_i n_i, n_i = -g_i / |g_i| where the raw
    density is positive and g_i . g_i > 0, else 0, g_i the world-space gradient of the raw density; raw = 0 at the samples `keep`
    drops.  With want_pres also the hidden pre-activations, and sigma and |g| of the kept rows."""
    dtype = params["emb"].dtype
    n, S = o.shape[0], t.shape[0]
    od, dd = o.to(dtype), d.to(dtype)
    index, M, ids, x32, _ = _ray_rows(params, o, d, od, dd, t, frame, offsets, scales, keep)
    xd = x32.to(dtype).requires_grad_(True)
    geo, pres = sigma_of(params, x32, xd, offsets, scales)
    sigma_rows = geo[:, 0]
    g_x, = torch.autograd.grad(sigma_rows.sum(), xd)
    g_p = points_backward(o, d, t, S, index, M, frame, g_x)
    sigma = torch.zeros(n * S, dtype=dtype)
    sigma[ids] = sigma_rows.detach()
    grad = torch.zeros(n * S, 3, dtype=dtype)
    grad[ids] = g_p
    gg = (grad * grad).sum(-1)
    use = (sigma > 0) & (gg > 0)
    nrm = torch.where(use[:, None], -grad / torch.sqrt(torch.where(use, gg, torch.ones_like(gg)))[:, None], torch.zeros_like(grad))
    w = composite_weights(sigma.view(n, S), t, dtype)
    out = w.sum(1), (w[..., None] * nrm.view(n, S, 3)).sum(1)
    return out + (pres, sigma_rows.detach(), g_p.norm(dim=1)) if want_pres else out


def render_rays(params, o, d, od, dd, t, frame, white, offsets, scales, keep=None):
    """R.render with the positions and the view directions carrying their derivative: od, dd are o, d (float32 values) in the
    parameters' dtype and may require grad, as may the parameters.  The forward values are R.render's."""
    dtype = params["emb"].dtype
    n, S = o.shape[0], t.shape[0]
    P = n * S
    index, M, ids, x32, xd = _ray_rows(params, o, d, od, dd, t, frame, offsets, scales, keep)
    raw = torch.zeros(P, 4, dtype=dtype)
    if M:
        geo, _ = sigma_of(params, x32, xd, offsets, scales)
        shd = sh4_differentiable(dd)
        sh = R.sh4(d, dtype) + (shd - shd.detach())
        rgb_raw, _ = R.mlp(torch.cat([geo, sh[ids // S]], dim=1), params["cw"], params["cb"])
        raw = R.raw_scatter(rgb_raw, geo[:, 0], index, M, P)
    return R.composite(raw.view(n, S, 4), t, white, dtype)
