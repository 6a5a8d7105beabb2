"""Restatement of the hash field's sampling (include/nerf_mi355x_sampling.h), in torch on the CPU: the yardstick
of tests/test_hashfield_sampling_cpu.py and tests/test_gpu_hashfield_sampling.py.  A helper, not a test; written from the formulas of
the header, not from any kernel, and it imports nothing of the package.

    fp32, the header's order   sample_importance, stratified, density_scatter: every operation one separately rounded torch op, the sums
                               sequential and left to right, so the kernels match them bit for bit
    float64                    sample_importance_f64: the reference's expressions (pdf = w' / sum w', cumsum, searchsorted(right),
                               the interpolation) for any counts, with the last bin reachable
    per-ray depths             points_rays, composite_rays, render_rays, coarse_weights: hashfield_reference's functions for depths
                               t [n,S] instead of one shared table; differentiable torch in the parameters' dtype
"""
import json
import os
import shutil

import torch

import hashfield_reference as R

U = R.U
EPS_W = 1e-5
REPO = R.REPO
SAMPLING_JSON = os.path.join(REPO, "profiles", "hashfield_sampling.json")


def _rows(x, n):
    """A shared table [k] as the same row for n rays; a table per ray [n,k] as it is."""
    return x[None, :].expand(n, x.shape[0]) if x.dim() == 1 else x


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def cdf_of(weights):
    """weights [n,Sc] float32 -> the K + 1 = Sc - 1 cdf values per ray, float32: the sequential sums of the header."""
    n, Sc = weights.shape
    K = Sc - 2
    assert K >= 1 and weights.dtype == torch.float32
    wp = weights[:, 1:Sc - 1] + torch.tensor(EPS_W, dtype=torch.float32)        # w'_i = fadd(w[i + 1], 1e-5f)
    total = wp[:, 0].clone()
    for i in range(1, K):                                                        # left to right, starting from w'_0
        total = total + wp[:, i]
    pdf = R.div_rn(wp, total[:, None].expand(n, K))
    cdf = torch.zeros(n, K + 1, dtype=torch.float32)
    for i in range(K):
        cdf[:, i + 1] = cdf[:, i] + pdf[:, i]
    return cdf


def sample_importance(weights, t_coarse, u):
    """weights [n,Sc], t_coarse [Sc] or [n,Sc], u [Sf] or [n,Sf] (any order), float32 -> (t_merged [n,Sc+Sf], t_fine [n,Sf]) float32,
    op by op in the header's order."""
    assert weights.dtype == t_coarse.dtype == u.dtype == torch.float32
    n, Sc = weights.shape
    K = Sc - 2
    t, uu = _rows(t_coarse, n), _rows(u, n)
    f32 = torch.float32
    cdf = cdf_of(weights)
    bins = 0.5 * (t[:, 1:] + t[:, :-1])                                          # K + 1 edges
    inds = (cdf[:, None, :] <= uu[:, :, None]).sum(-1)                           # #{cdf <= u}
    below, above = torch.clamp(inds - 1, 0, K), torch.clamp(inds, 0, K)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    denom = ca - cb
    denom = torch.where(denom < torch.tensor(EPS_W, dtype=f32), torch.ones_like(denom), denom)
    frac = R.div_rn(uu - cb, denom)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    fine = bb + frac * (ba - bb)
    assert fine.dtype == f32
    merged = torch.sort(torch.cat([t, fine], dim=1), dim=1).values
    return merged, fine


def sample_importance_f64(weights, t_coarse, u):
    """The reference's expressions in float64 from the same fp32 inputs -> (t_merged, t_fine, {"cdf", "bins", "inds"})."""
    n, Sc = weights.shape
    K = Sc - 2
    t, uu = _rows(t_coarse, n).double(), _rows(u, n).double().contiguous()
    wp = weights[:, 1:Sc - 1].double() + EPS_W
    pdf = wp / wp.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros(n, 1, dtype=torch.float64), torch.cumsum(pdf, -1)], -1)
    bins = 0.5 * (t[:, 1:] + t[:, :-1])
    inds = torch.searchsorted(cdf.contiguous(), uu, right=True)
    below, above = torch.clamp(inds - 1, 0, K), torch.clamp(inds, 0, K)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    denom = ca - cb
    denom = torch.where(denom < EPS_W, torch.ones_like(denom), denom)
    frac = (uu - cb) / denom
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    fine = bb + frac * (ba - bb)
    merged = torch.sort(torch.cat([t, fine], dim=1), dim=1).values
    return merged, fine, {"cdf": cdf, "bins": bins, "inds": inds, "denom": denom}


def stratified(t_table, jitter):
    """The CPU torch expression nerf_field_stratified_depths is bit-equal to: t_table [S], jitter [n,S] float32 -> [n,S]."""
    assert t_table.dtype == jitter.dtype == torch.float32
    mids = 0.5 * (t_table[1:] + t_table[:-1])
    lower = torch.cat([t_table[:1], mids])
    upper = torch.cat([mids, t_table[-1:]])
    return lower + (upper - lower) * jitter


def density_scatter(sigma_rows, index, n_rows, n_points, raw=None):
    """raw [n_points,4] = (0, 0, 0, sigma) at the rows' ids; the others keep what `raw` held (zeros if None)."""
    raw = torch.zeros(n_points, 4, dtype=sigma_rows.dtype) if raw is None else raw.clone()
    rows = torch.zeros(n_rows, 4, dtype=sigma_rows.dtype)
    rows[:, 3] = sigma_rows[:n_rows]
    raw[R.ids_of(index, n_rows)] = rows
    return raw


# ---- the field on depths per ray -------------------------------------------------------------------------------------------------------
def points_rays(o, d, t, index, n_rows, frame):
    """hashfield_reference.points for depths t [n,S]: row j -> the normalised position of point id (ray id // S, sample id % S)."""
    lo, hi, extent = frame
    S = t.shape[1]
    ids = R.ids_of(index, n_rows)
    ray, s = ids // S, ids % S
    p = o[ray] + d[ray] * t[ray, s][:, None]
    assert p.dtype == torch.float32
    c = torch.minimum(torch.maximum(p, lo[None]), hi[None])
    num = c - lo[None]
    return R.div_rn(num, torch.full_like(num, extent))


def composite_rays(raw, t, white, dtype):
    """hashfield_reference.composite for depths t [n,S] (float32) -> (rgb [n,3], depth [n], weights [n,S])."""
    n, S = raw.shape[0], raw.shape[1]
    t = t.to(torch.float32)
    delta = torch.cat([t[:, 1:] - t[:, :-1], torch.full((n, 1), 1e10, dtype=torch.float32)], dim=1).to(dtype)
    tt = t.to(dtype)
    T = torch.ones(n, dtype=dtype)
    rgb = torch.zeros(n, 3, dtype=dtype)
    depth = torch.zeros(n, dtype=dtype)
    wsum = torch.zeros(n, dtype=dtype)
    ws = []
    for k in range(S):
        alpha = 1.0 - torch.exp(-torch.relu(raw[:, k, 3]) * delta[:, k])
        w = T * alpha
        T = T * torch.clamp(1.0 - alpha, min=1e-10, max=1.0)
        col = 1.0 / (1.0 + torch.exp(-raw[:, k, :3]))
        rgb = rgb + w[:, None] * col
        depth = depth + w * tt[:, k]
        wsum = wsum + w
        ws.append(w)
    if white:
        rgb = rgb + (1.0 - wsum)[:, None]
    return rgb, depth, torch.stack(ws, dim=1)


def _kept(keep, P):
    index = None if keep is None else torch.nonzero(keep.reshape(-1)).reshape(-1).to(torch.int32)
    return index, (P if index is None else int(index.numel()))


def coarse_weights(params, o, d, t, frame, offsets, scales, keep=None):
    """The coarse pass in the parameters' dtype: the density network alone on the depths t [n,S] (or one table [S]), raw = 0 where
    `keep` is False, nerf_composite's weights [n,S]."""
    dtype = params["emb"].dtype
    n = o.shape[0]
    t = _rows(t, n).contiguous()
    S = t.shape[1]
    index, M = _kept(keep, n * S)
    raw = torch.zeros(n * S, 4, dtype=dtype)
    if M:
        x32 = points_rays(o, d, t, index, M, frame)
        geo, _ = R.mlp(R.hash_forward(x32, params["emb"], offsets, scales), params["sw"], params["sb"])
        raw = density_scatter(geo[:, 0], index, M, n * S)
    return composite_rays(raw.view(n, S, 4), t, 1, dtype)[2]


def render_rays(params, o, d, t, frame, white, offsets, scales, keep=None):
    """hashfield_reference.render on depths t [n,S] that are constants: differentiable with respect to the parameters.
    -> (rgb [n,3], depth [n])."""
    dtype = params["emb"].dtype
    n, S = t.shape
    index, M = _kept(keep, n * S)
    raw = torch.zeros(n * S, 4, dtype=dtype)
    if M:
        x32 = points_rays(o, d, t, index, M, frame)
        sh = R.sh4(d, dtype)
        rgb_raw, sigma, _ = R.field_rows(params, x32, sh[R.ids_of(index, M) // S], offsets, scales)
        raw = R.raw_scatter(rgb_raw, sigma, index, M, n * S)
    rgb, depth, _ = composite_rays(raw.view(n, S, 4), t, white, dtype)
    return rgb, depth


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def read_record():
    if not os.path.exists(SAMPLING_JSON):
        return {}
    with open(SAMPLING_JSON) as f:
        return json.load(f)


def record(key, stats):
    """Keep measured figures: merged into profiles/hashfield_sampling.json under `key` (hashfield_reference.parity_record's
    convention, its copy directory included)."""
    rec = read_record()
    rec[key] = stats
    os.makedirs(os.path.dirname(SAMPLING_JSON), exist_ok=True)
    with open(SAMPLING_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(SAMPLING_JSON, os.path.join(out, os.path.basename(SAMPLING_JSON)))
