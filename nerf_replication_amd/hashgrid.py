"""Multiresolution hash-grid encoding (instant-NGP) on the HIP kernels of csrc/nerf_hashgrid.hip.inc.

Public surface mirrors the reference's src/models/encoding/hashencoder/hashgrid.py:
    hash_encode(inputs, embeddings, offsets, per_level_scale, base_resolution, deterministic=False)
    HashEncoder(input_dim, num_levels, level_dim, per_level_scale, base_resolution, log2_hashmap_size, desired_resolution,
                deterministic=False)
    TriPlane(**kwargs)
fp32 throughout (the reference casts to half); other dtypes raise NotImplementedError.  CPU tensors raise
NerfLibraryError: there is no fallback.  The derivative with respect to the input is recomputed in the backward, nothing is stored in
the forward; double backward is not supported and raises.

deterministic=True sums the table gradient exactly in 64-bit fixed point (nerf_hashgrid_backward_deterministic, DESIGN.md section
2.12.1): the same bytes from run to run and under any permutation of the points, at 1.7 times the time of the fp32 atomics that the
default keeps (measured at 2^20 points).  The forward and the input gradient are the same kernels either way.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib

EPS = 1e-6
MAX_LEVELS = 32
INPUT_DIMS = (2, 3, 4)
LEVEL_DIMS = (1, 2, 4, 8)


def level_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size):
    """Row offsets of the levels, int32 [L+1]: level i has int(min(2^T, (res+1)^D) / 8) * 8 rows, res = ceil(H * s^i) in float64."""
    offsets, offset = [], 0
    for i in range(num_levels):
        res = int(math.ceil(base_resolution * float(per_level_scale) ** i))
        rows = min(2 ** log2_hashmap_size, (res + 1) ** input_dim)
        offsets.append(offset)
        offset += rows // 8 * 8
    offsets.append(offset)
    return np.array(offsets, dtype=np.int32)


def level_scales(num_levels, per_level_scale, base_resolution):
    """Grid scale of every level, float32 [L]: exp2(l * log2(s)) * H - 1 in float64, rounded once.  The host computes it (not the
    device's exp2f) so that the kernels and tests/hashgrid_reference.py cannot disagree about a cell."""
    log2_s = math.log2(float(per_level_scale))
    return np.array([2.0 ** (l * log2_s) * base_resolution - 1.0 for l in range(num_levels)], dtype=np.float64).astype(np.float32)


def _as_offsets(offsets):
    o = offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets)
    return np.ascontiguousarray(o, dtype=np.int32)


def _f32(t, what):
    if t.dtype != torch.float32:
        raise NotImplementedError(f"hash_encode: {what} must be float32 (got {t.dtype}); the encoder computes in fp32 only")
    return t


class _HashEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, embeddings, offsets, scales, deterministic):
        # inputs [B, D] in [0, 1], embeddings [offsets[-1], C], offsets int32 [L+1] and scales float32 [L] (ctypes host arrays)
        # -> [B, L*C]; deterministic: which entry sums the table gradient
        x = inputs.detach().contiguous()
        emb = embeddings.detach().contiguous()
        B, D = x.shape
        C, L = emb.shape[1], len(scales)
        if emb.shape[0] < offsets[L]:
            raise _lib.NerfLibraryError(f"hash_encode: embeddings has {emb.shape[0]} rows, the level table needs {offsets[L]}")
        out = torch.empty(B, L * C, dtype=torch.float32, device=x.device)
        _lib.call("nerf_hashgrid_forward", x, emb, B, D, C, L, offsets, scales, out)
        ctx.save_for_backward(x, emb)
        ctx.level_table = (offsets, scales)
        ctx.deterministic = deterministic
        return out

    @staticmethod
    @once_differentiable                # a double backward raises instead of returning zeros
    def backward(ctx, grad):
        x, emb = ctx.saved_tensors
        offsets, scales = ctx.level_table
        B, D = x.shape
        C, L = emb.shape[1], len(scales)
        grad = _f32(grad, "the output gradient").contiguous()
        grad_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        grad_emb = torch.zeros_like(emb) if ctx.needs_input_grad[1] else None
        if grad_emb is not None and ctx.deterministic:
            # the exact sum fills grad_emb; the existing entry is left the input gradient alone
            nbytes = _lib.call("nerf_hashgrid_deterministic_workspace_bytes", offsets[L] - offsets[0], C)
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            _lib.call("nerf_hashgrid_backward_deterministic", x, grad, B, D, C, L, offsets, scales, grad_emb, workspace, nbytes)
            if grad_x is not None:
                _lib.call("nerf_hashgrid_backward", x, emb, grad, B, D, C, L, offsets, scales, None, grad_x)
        else:
            _lib.call("nerf_hashgrid_backward", x, emb, grad, B, D, C, L, offsets, scales, grad_emb, grad_x)
        return grad_x, grad_emb, None, None, None


def _flag(deterministic, who):
    if not isinstance(deterministic, bool):
        raise ValueError(f"{who}: deterministic must be True or False (got {deterministic!r})")
    return deterministic


def hash_encode(inputs, embeddings, offsets, per_level_scale, base_resolution, deterministic=False):
    """inputs [B, D] in [0, 1], embeddings [offsets[-1], C], offsets [L+1] (int tensor or array) -> [B, L*C].  The gradient with
    respect to `inputs` is computed only if it requires grad, the one with respect to `embeddings` only if that does.
    deterministic=True: the gradient with respect to `embeddings` is the exact, order-independent sum (the module's docstring)."""
    _flag(deterministic, "hash_encode")
    if inputs.dim() != 2 or embeddings.dim() != 2:
        raise ValueError("hash_encode: inputs must be [B, D] and embeddings [rows, C]")
    _f32(inputs, "inputs")
    _f32(embeddings, "embeddings")
    if not inputs.is_cuda or not embeddings.is_cuda:
        raise _lib.NerfLibraryError("hash_encode needs tensors on a GPU (cuda) device; got a CPU tensor (there is no CPU fallback)")
    offsets = _as_offsets(offsets)
    L = offsets.shape[0] - 1
    if inputs.shape[0] == 0:            # nothing to encode (the C entry refuses an empty batch)
        return inputs.new_zeros(0, L * embeddings.shape[1])
    # the level tables as the host arrays the two entries take, made once for the forward and the backward
    scales = level_scales(L, per_level_scale, base_resolution)
    return _HashEncode.apply(inputs, embeddings, (ctypes.c_int32 * (L + 1))(*offsets.tolist()), (ctypes.c_float * L)(*scales.tolist()),
                             deterministic)


def normalize_to_bounds(xyz, wbounds):
    """The reference's normalisation: clamp into the box wbounds = (min xyz, max xyz), subtract the minimum, divide by the largest
    extent + 1e-6 (one divisor for all axes)."""
    lo, hi = wbounds[:3], wbounds[3:6]
    inputs = torch.clamp(xyz, min=lo, max=hi)
    inputs = inputs - lo[None]
    return inputs / ((hi - lo).max().item() + EPS)


class HashEncoder(nn.Module):
    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19,
                 desired_resolution=-1, deterministic=False, **kwargs):
        super().__init__()
        # a plain attribute (it may be changed between steps), not a parameter or buffer: the state_dict does not carry it
        self.deterministic = _flag(deterministic, "HashEncoder")
        if input_dim not in INPUT_DIMS or level_dim not in LEVEL_DIMS or not 1 <= num_levels <= MAX_LEVELS:
            raise ValueError(f"HashEncoder: input_dim in {INPUT_DIMS}, level_dim in {LEVEL_DIMS} and 1 <= num_levels <= {MAX_LEVELS} "
                             f"are built (got {input_dim}, {level_dim}, {num_levels})")
        # the finest resolution wanted at the last level, if given, overrides per_level_scale
        if desired_resolution != -1:
            per_level_scale = float(np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1)))
        self.input_dim = input_dim
        self.num_levels = num_levels
        self.level_dim = level_dim
        self.per_level_scale = per_level_scale
        self.log2_hashmap_size = log2_hashmap_size
        self.base_resolution = base_resolution
        self.output_dim = num_levels * level_dim
        self.out_dim = self.output_dim
        self.max_params = 2 ** log2_hashmap_size
        # a plain attribute, not a buffer: the state_dict holds "embeddings" alone, as the reference's does
        self.offsets = torch.from_numpy(level_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size))
        self.n_params = int(self.offsets[-1]) * level_dim
        self.embeddings = nn.Parameter(torch.zeros(int(self.offsets[-1]), level_dim))
        self.reset_parameters()

    def reset_parameters(self):
        self.embeddings.data.uniform_(-1e-4, 1e-4)

    def __repr__(self):
        return (f"HashEncoder: input_dim={self.input_dim} num_levels={self.num_levels} level_dim={self.level_dim} "
                f"H={self.base_resolution} params={tuple(self.embeddings.shape)}")

    def forward(self, xyz, wbounds=None, normalize=True):
        """xyz [..., input_dim] -> [..., num_levels * level_dim].  normalize=True maps world positions into [0, 1] with `wbounds`
        (normalize_to_bounds); normalize=False takes xyz as already in [0, 1]."""
        inputs = normalize_to_bounds(xyz, wbounds) if normalize else xyz
        prefix = list(inputs.shape[:-1])
        outputs = hash_encode(inputs.reshape(-1, self.input_dim), self.embeddings, self.offsets, self.per_level_scale,
                              self.base_resolution, self.deterministic)
        return outputs.view(prefix + [self.output_dim])


class TriPlane(nn.Module):
    """Three 2-D encoders on the (x, y), (y, z) and (x, z) planes of the normalised position, concatenated.  The keyword arguments
    are HashEncoder's (deterministic among them); input_dim is 2."""

    def __init__(self, **kwargs):
        super().__init__()
        kwargs = dict(kwargs, input_dim=2)
        self.xy_plane = HashEncoder(**kwargs)
        self.yz_plane = HashEncoder(**kwargs)
        self.xz_plane = HashEncoder(**kwargs)
        self.out_dim = self.xy_plane.out_dim * 3

    def forward(self, xyz, wbounds):
        inputs = normalize_to_bounds(xyz, wbounds)
        return torch.cat([self.xy_plane(inputs[..., [0, 1]], normalize=False),
                          self.yz_plane(inputs[..., [1, 2]], normalize=False),
                          self.xz_plane(inputs[..., [0, 2]], normalize=False)], dim=-1)
