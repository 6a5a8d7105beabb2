"""Restatement of the deterministic hash-grid table gradient (include/nerf_mi355x_hashgrid.h) on the CPU,
in integers: the yardstick of tests/test_hashgrid_deterministic_cpu.py and tests/test_gpu_hashgrid_deterministic.py.  The fp32 terms
come from the helpers of tests/hashgrid_reference.py (cells, corner_weight, corner_rows: the kernel's operations in the kernel's
order); the three passes are numpy int64 (np.maximum.at, np.add.at), whose result cannot depend on the order of the terms.  Written
from the description of the arithmetic, not from any code.
"""
import numpy as np
import torch

import hashgrid_reference as R

MAX_GUARD_BITS = 30
QNAN_BITS = 0x7FC00000


def guard_bits(B, D):
    """K = min(30, 39 - ceil(log2(B * 2^D))), the logarithm in integers."""
    return min(MAX_GUARD_BITS, 39 - (B * (1 << D) - 1).bit_length())


def workspace_bytes(rows, C):
    """int64 acc [rows*C] then uint32 emax [rows*C], rounded up to 256 bytes."""
    return (12 * rows * C + 255) // 256 * 256


def terms(x, offsets, scales, grad_out, C):
    """Every term t = fmul(w, grad_out[b, l*C + c]) of the call -> (element int64 [N], bits of t uint32 [N]); the element is
    (offsets[l] + row) * C + c.  x [B, D] and grad_out [B, L*C]: float32 CPU tensors."""
    x, grad_out = x.cpu(), grad_out.cpu()
    D, L = x.shape[1], len(offsets) - 1
    elems, bits = [], []
    ch = np.arange(C, dtype=np.int64)[None]
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        g, f = R.cells(x, scales[l])
        omf = 1 - f
        go = grad_out[:, l * C:(l + 1) * C]
        for idx in range(1 << D):
            rows = (R.corner_rows(g, idx, n, scales[l]) + int(offsets[l])).numpy().astype(np.int64)
            t = R.corner_weight(f, idx, omf)[:, None] * go                   # float32 [B, C]: one rounding
            elems.append((rows[:, None] * C + ch).reshape(-1))
            bits.append(t.contiguous().numpy().view(np.uint32).reshape(-1))
    return np.concatenate(elems), np.concatenate(bits)


def quantize(bits, emax, K):
    """The q of live terms (1 <= exponent <= 254) given the emax of their elements (>= the exponent, <= 254): int64."""
    bits = bits.astype(np.int64)
    e = (bits >> 23) & 0xFF
    m = (bits & 0x7FFFFF) | 0x800000
    s = emax - e
    assert (s >= 0).all()
    left = m << np.clip(K - s, 0, MAX_GUARD_BITS)
    right = np.where(s - K >= 24, 0, m >> np.clip(s - K, 0, 24))              # truncation of the magnitude
    return np.where(bits >> 31 != 0, -1, 1) * np.where(s <= K, left, right)


def exact_table_gradient(x, offsets, scales, grad_out, C, K, prev=None):
    """The table gradient of one call, accumulated into `prev` (float32 [rows, C], default zeros; rows = offsets[-1]).
    -> dict: grad float32 [rows, C]; emax int64 [rows, C] (0: no live term, 255: poisoned); acc int64 [rows, C];
             max_abs_acc: max |acc| (int); max_sum_abs_q: max over the elements of sum |q|, which bounds every partial sum in any
             order (float64)."""
    rows = int(offsets[-1])
    E = rows * C
    elem, bits = terms(x, offsets, scales, grad_out, C)
    e = ((bits >> 23) & 0xFF).astype(np.int64)
    emax = np.zeros(E, np.int64)
    np.maximum.at(emax, elem, e)
    top = emax[elem]
    live = (e >= 1) & (e <= 254) & (top < 255)
    q = quantize(bits[live], top[live], K)
    acc = np.zeros(E, np.int64)
    np.add.at(acc, elem[live], q)
    abs_acc = np.zeros(E, np.float64)                                         # (float64 holds 2^63 exactly enough for "< 2^63")
    np.add.at(abs_acc, elem[live], np.abs(q).astype(np.float64))
    out = np.zeros(E, np.float32) if prev is None else prev.detach().cpu().contiguous().numpy().reshape(-1).astype(np.float32, copy=True)
    assert out.shape == (E,)
    summed = (emax >= 1) & (emax <= 254)
    v = np.ldexp(acc[summed].astype(np.float32), (emax[summed] - 150 - K).astype(np.int32)).astype(np.float32)
    out[summed] = out[summed] + v                                             # one float32 add
    out.view(np.uint32)[emax == 255] = QNAN_BITS
    return {"grad": torch.from_numpy(out).view(rows, C), "emax": emax.reshape(rows, C), "acc": acc.reshape(rows, C),
            "max_abs_acc": int(np.abs(acc).max()), "max_sum_abs_q": float(abs_acc.max())}


def truncation_bound(count, emax, K):
    """count * 2^(emax - 150 - K) per element, float64 (0 where nothing is summed): what the right shifts can lose."""
    unit = np.ldexp(1.0, (np.clip(emax, 1, 254) - 150 - K).astype(np.int64))
    return np.where((emax >= 1) & (emax <= 254), count * unit, 0.0)
