"""CPU side of the geometry-output tests (tests/test_normals_cpu.py, tests/test_gpu_normals.py): the definitions of
include/nerf_mi355x.h ("geometry outputs") restated with torch autograd and float64 on the oracle's functions.

  g_i = grad_x raw sigma(x_i);  n_i = -g_i / |g_i| where raw sigma_i > 0 and g_i . g_i > 0, else 0;
  acc = sum_i w_i,  normal = sum_i w_i n_i  with the weights of oracle.transmittance_weights on relu(sigma).
"""
import torch

import nerf_oracle as orc


def sigma_and_gradient(sd, prefix, pts, dtype=torch.float32):
    """(raw sigma [P], d raw sigma / d x [P,3]) of the sub-model `prefix` ("model" / "model_fine") at pts [P,3]: torch.autograd.grad
    of oracle.nerf_mlp(...)[..., 3].sum() through oracle.freq_encode, in `dtype` (float64: on the fp32 weights and points).  The
    view direction does not reach sigma; its encoding is fed as zeros."""
    sub = {k: v.detach().to(dtype) for k, v in sd.items() if k.startswith(prefix + ".")}
    x = pts.detach().to(dtype).clone().requires_grad_(True)
    emb = torch.cat([orc.freq_encode(x, orc.XYZ_FREQS), torch.zeros(x.shape[0], 3 + 6 * orc.DIR_FREQS, dtype=dtype)], -1)
    sigma = orc.nerf_mlp(sub, prefix, emb)[..., 3]
    (g,) = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach(), g.detach()


def point_normals(sigma, grad):
    """n = -g / |g| where sigma > 0 and g . g > 0, else the zero vector, in float64."""
    g = grad.double()
    gg = (g * g).sum(-1, keepdim=True)
    has = (sigma.double()[..., None] > 0) & (gg > 0)
    return torch.where(has, -g / torch.sqrt(torch.where(has, gg, torch.ones_like(gg))), torch.zeros_like(g))


def composite_normals(raw, t, grad):
    """raw [n,S,4] (sigma = channel 3, pre-ReLU), t [n,S], grad [n,S,3] -> (normal [n,3], acc [n], weights [n,S]), float64."""
    sigma = raw[..., 3].double()
    _, w = orc.transmittance_weights(torch.relu(sigma), t.double())
    nrm = point_normals(sigma, grad)
    return (w[..., None] * nrm).sum(1), w.sum(-1), w


PLANAR_BIAS = 16.0


def planar_state_dict(sd, a, c, prefix="model_fine"):
    """A copy of `sd` whose sub-model `prefix` computes raw sigma(x) = a . x + c (its colour branch all zero): pts_linears.0 takes
    +x and -x from the three raw-input channels of the encoding into features 0..5 with bias 16 (positive for |x_i| < 16, so every
    ReLU passes them), layers 1..7 are the identity on those six features (layer 5's weights at input columns 63 + i: it reads
    [encoding | h4]), alpha_linear is (a/2, -a/2) with bias c.  The gradient is `a` exactly for dyadic a: every product is by +-1 or
    a_i / 2 and the two halves add up without rounding."""
    out = {k: v.detach().clone() for k, v in sd.items()}
    for k in orc.SUBMODEL_KEYS:
        out[f"{prefix}.{k}"] = torch.zeros_like(out[f"{prefix}.{k}"])
    w0, b0 = out[f"{prefix}.pts_linears.0.weight"], out[f"{prefix}.pts_linears.0.bias"]
    for i in range(3):
        w0[i, i], w0[3 + i, i] = 1.0, -1.0
    b0[:6] = PLANAR_BIAS
    for layer in range(1, 8):
        w = out[f"{prefix}.pts_linears.{layer}.weight"]
        col0 = 63 if layer == 5 else 0
        for i in range(6):
            w[i, col0 + i] = 1.0
    wa = out[f"{prefix}.alpha_linear.weight"]
    for i in range(3):
        wa[0, i], wa[0, 3 + i] = 0.5 * a[i], -0.5 * a[i]
    out[f"{prefix}.alpha_linear.bias"][0] = c
    return out


def parse_ply(data):
    """Minimal reader of write_ply's files: bytes -> (vertex property names, vertex rows [V, len(names)] float32, faces [T,3])."""
    import numpy as np
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    names, n_v, n_f, element = [], 0, 0, None
    for ln in lines[2:]:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] == "element":
            element = tok[1]
            if element == "vertex":
                n_v = int(tok[2])
            else:
                assert element == "face"
                n_f = int(tok[2])
        elif tok[0] == "property" and element == "vertex":
            assert tok[1] == "float"
            names.append(tok[2])
        elif tok[0] == "property":
            assert tok[1:] == ["list", "uchar", "int", "vertex_indices"]
    v = np.frombuffer(body, dtype="<f4", count=n_v * len(names)).reshape(n_v, len(names))
    rec = np.frombuffer(body, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=n_f, offset=v.nbytes)
    assert v.nbytes + rec.nbytes == len(body) and (rec["n"] == 3).all()
    return names, v, rec["i"]


def geometry_pipeline(sd, o, d, dtype):
    """The deterministic hierarchical render's geometry outputs on the CPU, both networks (encoding, MLPs and the density
    gradient) and the sampler in `dtype` on the fp32 rays, weights and tables; the compositing sums are float64 either way
    (composite_normals).  -> dict(normal [n,3], acc [n], bins (below, above) of the inverse-CDF sampler)."""
    import ray_grad_common as RG
    n = o.shape[0]
    o_, d_ = o.detach().to(dtype), d.detach().to(dtype)
    t_c = orc.stratified_t().to(dtype)[None].expand(n, orc.N_SAMPLES).contiguous()
    u = orc.fine_u().to(dtype).expand(n, orc.N_IMPORTANCE).contiguous()
    pts_c = orc.points_on_rays(o_, d_, t_c)
    sigma_c, _ = sigma_and_gradient(sd, "model", pts_c.reshape(-1, 3), dtype)
    sigma_c = torch.relu(sigma_c.reshape(n, orc.N_SAMPLES))
    below, above = RG.sampler_bins(sigma_c, t_c, u)
    _, w = orc.transmittance_weights(sigma_c, t_c)
    w = w[:, 1:-1] + 1e-5
    cdf = torch.cumsum(w / torch.sum(w, -1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
    mids = 0.5 * (t_c[:, 1:] + t_c[:, :-1])
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(mids, 1, below), torch.gather(mids, 1, above)
    denom = ca - cb
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t_f = bb + (u - cb) / denom * (ba - bb)
    t_s, _ = torch.sort(torch.cat([t_c, t_f], 1), dim=-1)
    pts = orc.points_on_rays(o_, d_, t_s)
    sigma, g = sigma_and_gradient(sd, "model_fine", pts.reshape(-1, 3), dtype)
    S = t_s.shape[1]
    raw = torch.zeros(n, S, 4, dtype=dtype)
    raw[..., 3] = sigma.reshape(n, S)
    normal, acc, _ = composite_normals(raw, t_s, g.reshape(n, S, 3))
    return {"normal": normal, "acc": acc, "bins": (below, above)}
