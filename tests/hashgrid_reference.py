"""Restatement of the multiresolution hash-grid encoding, in torch: the yardstick of
tests/test_hashgrid_cpu.py and tests/test_gpu_hashgrid.py and, run on the GPU, the baseline of tools/time_hashgrid.py (what a user
would write without the HIP kernels: gathers and index_add_).  Written from the description of the semantics, not from any code.

    level table        level_offsets, level_scales, level_strides      (host, Python ints and float64)
    fp32, fixed order  forward_f32: the kernel's forward bit for bit   (same operations in the same order, each rounded on its own)
                       backward_f32: the gradients as gather + index_add_ (any order: a baseline, not a yardstick)
    float64 truth      truth_f64: forward and both gradients from the fp32 cell and fraction, everything after them in float64, with
                       the number of terms and the sum of their absolute values per element (the error bounds of the GPU tests)
                       forward_autograd_f64: the same forward as differentiable torch, to pin truth_f64's analytic gradients

uint32 arithmetic is emulated in int64 modulo 2^32: for inputs in [0, 1] a grid coordinate stays below 2^21 and a stride below 2^32,
so a product stays below 2^53 and is reduced exactly.
"""
import math

import numpy as np
import torch

PRIMES = (1, 19349663, 83492791, 25165843)
M32 = (1 << 32) - 1


# ---- level table (host) ------------------------------------------------------------------------------------------------------------
def effective_scale(num_levels, per_level_scale, base_resolution, desired_resolution=-1):
    if desired_resolution != -1:
        return float(np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1)))
    return per_level_scale


def level_offsets(D, L, s, H, T):
    """Exclusive prefix sum of the level sizes n_i = int(min(2^T, (res+1)^D) / 8) * 8, res = ceil(H * s^i) -> list of L+1 ints."""
    offsets = [0]
    for i in range(L):
        res = int(math.ceil(H * float(s) ** i))
        offsets.append(offsets[-1] + int(min(2 ** T, (res + 1) ** D) / 8) * 8)
    return offsets


def level_scales(L, s, H):
    """float32(exp2(l * log2(s)) * H - 1): float64 on the host, rounded once."""
    return [np.float32(2.0 ** (l * math.log2(float(s))) * H - 1.0) for l in range(L)]


def level_strides(n, scale, D):
    """The index walk of one level in uint32 -> (hashed, strides used so far, final stride).  resolution = uint32(ceil(scale)) + 1."""
    res1 = (int(math.ceil(float(np.float32(scale)))) + 1 + 1) & M32
    stride, strides = 1, []
    for _ in range(D):
        if stride > n:
            break
        strides.append(stride)
        stride = (stride * res1) & M32
    return stride > n, strides, stride


# ---- cell, weights, rows -----------------------------------------------------------------------------------------------------------
def cells(x, scale):
    """x [B, D] float32 -> g int64 [B, D] (the cell), f float32 [B, D] (the fraction); multiply and add rounded separately."""
    assert x.dtype == torch.float32
    pos = x * float(np.float32(scale))           # (a Python float that is exactly the float32: torch multiplies in float32)
    pos = pos + 0.5
    fl = torch.floor(pos)
    return fl.to(torch.int64), pos - fl


def corner_rows(g, idx, n, scale):
    """Row inside the level of corner `idx` of the cells g [B, D] -> int64 [B]."""
    D = g.shape[1]
    hashed, strides, _ = level_strides(n, scale, D)
    gc = [(g[:, d] + ((idx >> d) & 1)) & M32 for d in range(D)]
    index = torch.zeros_like(gc[0])
    if hashed:
        for d in range(D):
            index = index ^ ((gc[d] * PRIMES[d]) & M32)
    else:
        for d in range(D):
            index = (index + gc[d] * strides[d]) & M32
    return index % n


def corner_weight(f, idx, one_minus_f=None):
    """1 * prod_d (bit d of idx ? f_d : 1 - f_d), d ascending, in f's dtype."""
    omf = 1 - f if one_minus_f is None else one_minus_f
    w = torch.ones_like(f[:, 0])
    for d in range(f.shape[1]):
        w = w * (f[:, d] if (idx >> d) & 1 else omf[:, d])
    return w


# ---- fp32, fixed order -------------------------------------------------------------------------------------------------------------
def forward_f32(x, emb, offsets, scales):
    """out[b, l*C + c] = sum over idx ascending, from 0, of w * emb[offsets[l] + row, c]: float32 [B, L*C]."""
    B, D = x.shape
    C, L = emb.shape[1], len(offsets) - 1
    out = torch.empty(B, L * C, dtype=torch.float32, device=x.device)
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        g, f = cells(x, scales[l])
        omf = 1 - f
        acc = torch.zeros(B, C, dtype=torch.float32, device=x.device)
        for idx in range(1 << D):
            rows = corner_rows(g, idx, n, scales[l]) + int(offsets[l])
            acc = acc + corner_weight(f, idx, omf)[:, None] * emb[rows]
        out[:, l * C:(l + 1) * C] = acc
    return out


def backward_f32(x, emb, offsets, scales, grad_out, want_emb=True, want_x=True):
    """The gradients in float32 with gathers and index_add_ -> (grad_emb or None, grad_x or None)."""
    B, D = x.shape
    C, L = emb.shape[1], len(offsets) - 1
    grad_emb = torch.zeros_like(emb) if want_emb else None
    grad_x = torch.zeros_like(x) if want_x else None
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        scale = float(np.float32(scales[l]))
        g, f = cells(x, scales[l])
        omf = 1 - f
        go = grad_out[:, l * C:(l + 1) * C]
        rows = [corner_rows(g, idx, n, scales[l]) + int(offsets[l]) for idx in range(1 << D)]
        if want_emb:
            for idx in range(1 << D):
                grad_emb.index_add_(0, rows[idx], corner_weight(f, idx, omf)[:, None] * go)
        if want_x:
            e = [emb[r] for r in rows]
            for d in range(D):
                for idx in range(1 << D):
                    if (idx >> d) & 1:
                        continue
                    w = torch.full_like(f[:, 0], scale)
                    for a in range(D):
                        if a != d:
                            w = w * (f[:, a] if (idx >> a) & 1 else omf[:, a])
                    grad_x[:, d] += (go * (w[:, None] * (e[idx | (1 << d)] - e[idx]))).sum(dim=1)
    return grad_emb, grad_x


# ---- float64 truth -----------------------------------------------------------------------------------------------------------------
def truth_f64(x, emb, offsets, scales, grad_out=None):
    """Forward and gradients in float64 from the float32 cell and fraction (so the truth never sits in another cell than the kernel).
    -> dict: out [B, L*C]; with grad_out also
         grad_emb, grad_emb_abs (sum of |term|), grad_emb_count (number of terms) per element of emb, term = w * grad_out
         grad_x, grad_x_abs, grad_x_count per element of x, term = grad_out * scale * prod_(a != d) factor_a * (emb[right] - emb[left])"""
    B, D = x.shape
    C, L = emb.shape[1], len(offsets) - 1
    emb64 = emb.double()
    res = {"out": torch.empty(B, L * C, dtype=torch.float64, device=x.device)}
    if grad_out is not None:
        go_all = grad_out.double()
        for k in ("grad_emb", "grad_emb_abs", "grad_emb_count"):
            res[k] = torch.zeros(emb.shape, dtype=torch.float64, device=x.device)
        for k in ("grad_x", "grad_x_abs", "grad_x_count"):
            res[k] = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        scale = float(np.float32(scales[l]))
        g, f32 = cells(x, scales[l])
        f = f32.double()
        rows = [corner_rows(g, idx, n, scales[l]) + int(offsets[l]) for idx in range(1 << D)]
        e = [emb64[r] for r in rows]
        acc = torch.zeros(B, C, dtype=torch.float64, device=x.device)
        for idx in range(1 << D):
            acc = acc + corner_weight(f, idx)[:, None] * e[idx]
        res["out"][:, l * C:(l + 1) * C] = acc
        if grad_out is None:
            continue
        go = go_all[:, l * C:(l + 1) * C]
        for idx in range(1 << D):
            term = corner_weight(f, idx)[:, None] * go
            res["grad_emb"].index_add_(0, rows[idx], term)
            res["grad_emb_abs"].index_add_(0, rows[idx], term.abs())
            res["grad_emb_count"].index_add_(0, rows[idx], torch.ones_like(term))
        for d in range(D):
            for idx in range(1 << D):
                if (idx >> d) & 1:
                    continue
                w = torch.full_like(f[:, 0], scale)
                for a in range(D):
                    if a != d:
                        w = w * (f[:, a] if (idx >> a) & 1 else 1 - f[:, a])
                term = go * (w[:, None] * (e[idx | (1 << d)] - e[idx]))
                res["grad_x"][:, d] += term.sum(dim=1)
                res["grad_x_abs"][:, d] += term.abs().sum(dim=1)
                res["grad_x_count"][:, d] += C
    return res


def forward_autograd_f64(x, x64, emb64, offsets, scales):
    """The forward as differentiable float64 torch: x (float32) fixes the cell and the value of the fraction, x64 (float64, requires
    grad, equal to x) carries the derivative d pos / d x = scale; emb64 may require grad."""
    B, D = x.shape
    C, L = emb64.shape[1], len(offsets) - 1
    outs = []
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        scale = float(np.float32(scales[l]))
        g, f32 = cells(x, scales[l])
        f = f32.double() + (x64 - x64.detach()) * scale
        acc = 0
        for idx in range(1 << D):
            acc = acc + corner_weight(f, idx)[:, None] * emb64[corner_rows(g, idx, n, scales[l]) + int(offsets[l])]
        outs.append(acc)
    return torch.cat(outs, dim=1)


# ---- test inputs -------------------------------------------------------------------------------------------------------------------
def boundary_points(H):
    """float32 x for which the level-0 position x * (H - 1) + 0.5, computed in float32, is exactly an integer: the point sits on a
    cell boundary (fraction exactly 0).  Candidates (j + 0.5) / (H - 1) and their float32 neighbours, kept where the product lands."""
    j = torch.arange(H - 1, dtype=torch.float64)
    c = ((j + 0.5) / (H - 1)).float()
    cand = torch.cat([c, torch.nextafter(c, torch.ones_like(c)), torch.nextafter(c, torch.zeros_like(c))])
    pos = cand * float(H - 1) + 0.5
    return cand[pos == torch.floor(pos)]


def make_inputs(B, D, H, seed):
    """B points in [0, 1]^D (float32): uniform random; from 3 points on, row 0 is exact 0, row 1 exact 1, and the next rows (up to 2H,
    as many as fit) have axes 0 and 1 exactly on level-0 cell boundaries."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=gen, dtype=torch.float32)
    if B >= 3:
        x[0] = 0.0
        x[1] = 1.0
        xb = boundary_points(H)
        m = min(B - 2, 2 * H)
        xb = xb[torch.arange(m) % xb.shape[0]]
        x[2:2 + m, 0] = xb
        x[2:2 + m, 1] = xb.flip(0)
    return x
