"""Restatement of the fused MLP's exact weight and bias gradients (include/nerf_mi355x_nn_exact.h) on the
CPU, in integers: the yardstick of tests/test_fused_mlp_exact_cpu.py and tests/test_gpu_fused_mlp_exact.py.  Written from the
description of the arithmetic, not from any code.  A term is one float32 product (or, for a bias, one float32 value); everything
after it is int64: the column maxima are unsigned maxima of bit patterns, the quantisation is shifts, the sum is an int64 sum over
the rows, whose result cannot depend on their order.

Why torch tensors and not numpy arrays: a weight gradient has B * n_out * n_in terms (226 million for 42 -> 128 x 4 -> 3 at
B = 4113, the largest GPU case), every one of which passes through a dozen int64 operations; numpy runs them on one core and takes
tens of seconds where a GPU test has a few, torch spreads the same element-wise integer operations over the CPU's cores.  The
operations are the same kind (shifts, masks, where, an int64 sum over the row axis) and nothing floating-point happens after the
term is formed; finish() is numpy.  For the same reason the quantisation is written with one shift instead of the description's
two cases (_quantize explains the identity); tests/test_fused_mlp_exact_cpu.py holds it to hashgrid_exact_reference.quantize, the
numpy function of the hash-grid restatement that states the two cases literally, on 50 000 random live terms.
"""
import numpy as np
import torch

MAX_GUARD_BITS = 30
QNAN_BITS = 0x7FC00000
SLAB_TERMS = 1 << 23                      # terms formed at a time


def guard_bits(B):
    """K = min(30, 39 - ceil(log2(B))), the logarithm in integers."""
    return min(MAX_GUARD_BITS, 39 - (B - 1).bit_length())


def layer_shapes(in_dim, width, n_hidden, out_dim):
    """[(n_out, n_in)] of the hidden layers in order, then the output layer."""
    return [(width if i < n_hidden else out_dim, width if i else in_dim) for i in range(n_hidden + 1)]


def workspace_bytes(in_dim, width, n_hidden, out_dim):
    """int64 accumulators of every weight and bias element, then the uint32 column maxima of x, the save blocks and the gsave blocks,
    rounded up to 256 bytes."""
    shapes = layer_shapes(in_dim, width, n_hidden, out_dim)
    acc = sum(o * k + o for o, k in shapes)
    maxima = sum(k for _, k in shapes) + sum(o for o, _ in shapes)
    return (8 * acc + 4 * maxima + 255) // 256 * 256


def bits_of(t):
    """float32 tensor -> its bit patterns as non-negative int64."""
    return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def exponent(bits):
    return (bits >> 23) & 0xFF


def column_max(a):
    """a float32 [B, n] -> int64 [n]: the unsigned maximum over the rows of the bit patterns with the sign cleared."""
    return (bits_of(a) & 0x7FFFFFFF).max(0).values


def product_exponent(A, H):
    """The biased exponent field of fmul(A[o], H[k]) -> int64 [n_out, n_in]; A, H: sign-cleared bit patterns."""
    a = A.to(torch.int32).view(torch.float32)
    h = H.to(torch.int32).view(torch.float32)
    return exponent(bits_of(a[:, None] * h[None, :]))


def _quantize(bits, emax, K):
    """-> (q, live, s): the q of every term given the emax of its element (broadcast), int64, 0 for a term that is not live (exponent
    0 or 255); which terms are live; s = emax - exponent, which must not be negative for a live term.
    m << (K - s) for s <= K and m >> (s - K) beyond it are one expression: m * 2^30 has 30 zero bits at its low end, so shifting it
    right by 30 - K + s (at most 30 when s <= K) loses nothing, and by more it truncates the magnitude as the right shift of m does;
    from 54 on nothing is left of the 54-bit m * 2^30, which is the rule '24 or more gives 0'."""
    e = exponent(bits)
    live = (e != 0) & (e != 255)
    s = emax - e
    mag = (((bits & 0x7FFFFF) | 0x800000) << MAX_GUARD_BITS) >> (s + (MAX_GUARD_BITS - K)).clamp_(0, 63)
    return torch.where(bits >> 31 != 0, -mag, mag).mul_(live), live, s


def quantize(bits, emax, K):
    return _quantize(bits, emax, K)[0]


def finish(acc, emax, K, prev):
    """acc, emax int64 [...]; prev float32 [...] -> float32 [...]: untouched where emax == 0, quiet NaN where emax == 255, else
    prev + ldexp(float32(acc), emax - 150 - K), one float32 addition."""
    out = prev.detach().cpu().to(torch.float32).contiguous().clone().numpy()
    acc, emax = acc.numpy(), emax.numpy()
    summed = (emax >= 1) & (emax <= 254)
    v = np.ldexp(acc[summed].astype(np.float32), (emax[summed] - 150 - K).astype(np.int32)).astype(np.float32)
    out[summed] = out[summed] + v
    out.view(np.uint32)[emax == 255] = QNAN_BITS
    return torch.from_numpy(out)


def exact_weight_gradient(dz, inp, K, prev=None):
    """dz float32 [B, n_out], inp float32 [B, n_in] (CPU) -> dict: grad float32 [n_out, n_in] = prev (default zeros) with the call's
    exact sum added; emax, acc int64 [n_out, n_in]; max_abs_acc (int); invariant (bool): no live term's exponent exceeded the
    emax of an element that is summed; count int64 [n_out, n_in]: live terms per element."""
    dz, inp = dz.detach().cpu().contiguous(), inp.detach().cpu().contiguous()
    B, n_out = dz.shape
    n_in = inp.shape[1]
    emax = product_exponent(column_max(dz), column_max(inp))
    acc = torch.zeros(n_out, n_in, dtype=torch.int64)
    count = torch.zeros(n_out, n_in, dtype=torch.int64)
    invariant = True
    top = torch.where(emax == 255, torch.full_like(emax, 1 << 20), emax)    # (a poisoned element: its sum is never used)
    step = max(1, SLAB_TERMS // (n_out * n_in))
    rows_live = (bits_of(dz) & 0x7FFFFFFF).ne(0).any(1)                      # a row whose dz are all zero forms only null terms
    dz_live, inp_live = dz[rows_live], inp[rows_live]
    for r in range(0, dz_live.shape[0], step):
        t = dz_live[r:r + step, :, None] * inp_live[r:r + step, None, :]     # float32: one rounding per term
        q, live, s = _quantize(bits_of(t), top[None], K)
        invariant = invariant and int(s.mul_(live).min()) >= 0
        acc += q.sum(0)
        count += live.sum(0)
    acc = torch.where(emax == 255, torch.zeros_like(acc), acc)
    prev = torch.zeros(n_out, n_in) if prev is None else prev
    return {"grad": finish(acc, emax, K, prev), "emax": emax, "acc": acc, "max_abs_acc": int(acc.abs().max()), "invariant": invariant,
            "count": count}


def exact_bias_gradient(dz, K, prev=None):
    """dz float32 [B, n_out] -> dict as above for the bias: the terms are the dz themselves, emax the exponent of the column maximum."""
    dz = dz.detach().cpu().contiguous()
    emax = exponent(column_max(dz))
    bits = bits_of(dz)
    e = exponent(bits)
    live = (e >= 1) & (e <= 254)
    top = torch.where(emax == 255, torch.full_like(emax, 1 << 20), emax)
    acc = quantize(bits, top[None], K).sum(0)
    acc = torch.where(emax == 255, torch.zeros_like(acc), acc)
    prev = torch.zeros(dz.shape[1]) if prev is None else prev
    return {"grad": finish(acc, emax, K, prev), "emax": emax, "acc": acc, "max_abs_acc": int(acc.abs().max()), "invariant": True,
            "count": live.sum(0)}


def layer_operands(x, save, gsave, B, in_dim, width, n_hidden, out_dim):
    """The (dz_i, in_i) of every layer from the kernel's own flat save and gsave buffers (CPU float32)."""
    plane = B * width
    ops = []
    for i, (n_out, n_in) in enumerate(layer_shapes(in_dim, width, n_hidden, out_dim)):
        dz = gsave[i * plane:i * plane + B * n_out].view(B, n_out)
        inp = x.view(B, in_dim) if i == 0 else save[(i - 1) * plane:i * plane].view(B, width)
        ops.append((dz, inp))
    return ops


def error_bound(dz, inp, emax, K, truth):
    """The derived bound per element, float64: 2^-24 * sum_p |dz * in| + B * 2^(emax - 150 - K) + 2^-24 * |truth| (term formation,
    truncation, the final rounding); inp None: a bias, whose terms are not formed.  Elements that are not summed: 0."""
    B = dz.shape[0]
    u = 2.0 ** -24
    form = 0.0 if inp is None else u * (dz.double().abs().T @ inp.double().abs())
    unit = torch.ldexp(torch.ones((), dtype=torch.float64), (emax.clamp(1, 254) - 150 - K))
    bound = form + B * unit + u * truth.abs()
    return torch.where((emax >= 1) & (emax <= 254), bound, torch.zeros((), dtype=torch.float64))
