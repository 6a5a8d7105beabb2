"""The deformation field of a dynamic scene on the HIP kernels of csrc/nerf_deform.hip.inc.

Public surface mirrors DNeRFNGP of the reference's src/models/encoding/hashencoder/hashgrid.py:
    DNeRFNGP(num_frames, feat_dim=64, reso=256, **hash_encoder_kwargs)
        encoder           a 3-D HashEncoder
        feat              nn.ParameterList of three [3, feat_dim, num_frames, reso] tables, 0.1 * randn
        forward(x [..., 4], wbounds)                 normalise, warp by the frame number in the last column, encode
        compute_delta(xyz01 [..., 3], t [..., 1])    the offset, differentiable with respect to feat
        compute_tv_loss(xyz [B,N,3], t [B,N,1], wbounds) -> [B,1]
State-dict keys: encoder.embeddings, feat.0, feat.1, feat.2 (a reference checkpoint of that module loads).  num_frames replaces the
reference's cfg.num_frames.  Every formula is in include/nerf_mi355x_deform.h.  The canonical frame is decided per point (a frame
number of exactly 0 leaves the position as it is), where the reference decides for the whole batch from its first point; the two
coincide for a batch that is all canonical or has no canonical point.

The kernels read the tables channel-innermost (one tap = one 256-byte row); the module keeps that packed copy and remakes it when a
table was written (the parameters' _version), so inference packs once.  fp32 only; CPU tensors raise NerfLibraryError: there is no
fallback.  The gradients with respect to the positions and the frame numbers are not built: inputs that require grad are refused.
The table gradient is summed by fp32 atomics; double backward raises.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .hashgrid import HashEncoder, hash_encode, normalize_to_bounds

FEAT_DIM = 64                       # channels: one wave's width (the reference hard-codes it)
MAX_SAMPLES = 192


def packed_floats(num_frames, reso):
    n = _lib.call("nerf_deform_packed_bytes", FEAT_DIM, int(num_frames), int(reso))
    if n < 0:
        raise ValueError(f"deformation field: num_frames >= 2, reso >= 2 and 9 * num_frames * reso * 64 <= 2^31 - 1 are built "
                         f"(got {num_frames}, {reso})")
    return n // 4


def pack_tables(feat, num_frames, reso):
    """Three contiguous cuda tables [3, 64, T, R] -> packed [9 * T * R * 64] (nerf_deform_pack)."""
    packed = torch.empty(packed_floats(num_frames, reso), dtype=torch.float32, device=feat[0].device)
    _lib.call("nerf_deform_pack", list(feat), FEAT_DIM, num_frames, reso, packed)
    return packed


class _Deform(torch.autograd.Function):
    """(feat0, feat1, feat2 -- the parameters, for autograd), packed, x [M,3], time [n], index, M, n, S, want -> x_warped [M,3]
    (want = "warp") or delta [M,3] (want = "delta"): nerf_deform_forward.  The backward recomputes everything from x and the
    tables: nerf_deform_backward into a zeroed packed gradient, nerf_deform_unpack_grad into the three gradients."""

    @staticmethod
    def forward(ctx, f0, f1, f2, packed, x, time, index, M, n, S, want):
        T, R = f0.shape[2], f0.shape[3]
        out = torch.empty(M, 3, dtype=torch.float32, device=x.device)
        warp = want == "warp"
        _lib.call("nerf_deform_forward", x, time, index, M, n, S, packed, FEAT_DIM, T, R, out if warp else None, None if warp else out)
        ctx.save_for_backward(packed, x, time)
        ctx.index, ctx.sizes, ctx.warp = index, (M, n, S, T, R), warp
        return out

    @staticmethod
    @once_differentiable                # a double backward raises instead of returning zeros
    def backward(ctx, g):
        packed, x, time = ctx.saved_tensors
        M, n, S, T, R = ctx.sizes
        if g.dtype != torch.float32:
            raise NotImplementedError(f"deformation field: the output gradient must be float32 (got {g.dtype})")
        g = g.contiguous()
        g_packed = torch.zeros_like(packed)
        _lib.call("nerf_deform_backward", x, time, ctx.index, M, n, S, packed, FEAT_DIM, T, R, g if ctx.warp else None,
                  None if ctx.warp else g, g_packed)
        grads = [torch.empty(3, FEAT_DIM, T, R, dtype=torch.float32, device=x.device) for _ in range(3)]
        _lib.call("nerf_deform_unpack_grad", g_packed, FEAT_DIM, T, R, grads)
        return (*grads, None, None, None, None, None, None, None, None)


class DNeRFNGP(nn.Module):
    def __init__(self, num_frames, feat_dim=FEAT_DIM, reso=256, **kwargs):
        super().__init__()
        if feat_dim != FEAT_DIM:
            raise ValueError(f"DNeRFNGP: feat_dim = {FEAT_DIM} is built (one wave's width; the reference hard-codes it), got {feat_dim!r}")
        for name, v in (("num_frames", num_frames), ("reso", reso)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 2:
                raise ValueError(f"DNeRFNGP: {name} must be an int >= 2, got {v!r}")
        if 9 * num_frames * reso * FEAT_DIM > 2 ** 31 - 1:
            raise ValueError(f"DNeRFNGP: 9 * num_frames * reso * 64 must be at most 2^31 - 1 (got {num_frames}, {reso})")
        if kwargs.get("input_dim", 3) != 3:
            raise ValueError("DNeRFNGP: the encoder is 3-D (input_dim = 3)")
        if kwargs.get("deterministic", False):
            raise NotImplementedError("DNeRFNGP(deterministic=True) is not built: the deformation tables' gradient is summed by "
                                      "atomics, so the promise of identical bytes would be false")
        self.num_frames, self.feat_dim, self.reso = num_frames, feat_dim, reso
        self.encoder = HashEncoder(**kwargs)
        self.feat = nn.ParameterList([nn.Parameter(0.1 * torch.randn(3, feat_dim, num_frames, reso)) for _ in range(3)])
        self.out_dim = self.encoder.out_dim
        self._packed = None

    # HashField reads these of its encoder
    @property
    def input_dim(self):
        return 3

    @property
    def deterministic(self):
        return self.encoder.deterministic

    def _check_tables(self):
        for i, f in enumerate(self.feat):
            if f.dtype != torch.float32:
                raise NotImplementedError(f"DNeRFNGP: fp32 only (feat.{i} is {f.dtype})")
            if tuple(f.shape) != (3, self.feat_dim, self.num_frames, self.reso):
                raise ValueError(f"DNeRFNGP: feat.{i} must be [3, {self.feat_dim}, {self.num_frames}, {self.reso}], got {tuple(f.shape)}")
        for f in self.feat:
            if not f.is_cuda:
                raise _lib.NerfLibraryError("DNeRFNGP needs its tables on a GPU (cuda) device; got a CPU tensor (there is no CPU fallback)")

    def packed(self):
        """The tables in the kernels' layout, remade when a table was written (an optimizer step, a loaded checkpoint, .to())."""
        self._check_tables()
        key = tuple((f.data_ptr(), f._version) for f in self.feat)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, pack_tables([f.detach().contiguous() for f in self.feat], self.num_frames, self.reso))
        return self._packed[1]

    def _apply_field(self, x, time, index, M, n, S, want):
        """x [M,3] contiguous in [0,1], time [n] per ray -> x_warped or delta [M,3]; differentiable with respect to feat when a
        table requires grad and grad mode is on, otherwise the one forward launch."""
        packed = self.packed()
        if torch.is_grad_enabled() and any(f.requires_grad for f in self.feat):
            return _Deform.apply(*self.feat, packed, x, time, index, M, n, S, want)
        out = torch.empty(M, 3, dtype=torch.float32, device=x.device)
        warp = want == "warp"
        _lib.call("nerf_deform_forward", x, time, index, M, n, S, packed, FEAT_DIM, self.num_frames, self.reso,
                  out if warp else None, None if warp else out)
        return out

    def warp(self, x, time, index=None, n_rays=None, n_samples=1):
        """Rows x [M,3] in [0,1] of the points `index` (None: all, in order) of n_rays rays with n_samples samples each, time
        [n_rays] -> the warped positions [M,3] (what HashField puts between nerf_field_points and hash_encode)."""
        n = x.shape[0] if n_rays is None else n_rays
        return self._apply_field(x, time, index, x.shape[0], n, n_samples, "warp")

    def _check_inputs(self, xyz, t, who):
        if not isinstance(xyz, torch.Tensor) or not isinstance(t, torch.Tensor) or xyz.shape[-1:] != (3,) or t.shape[-1:] != (1,) or \
                xyz.shape[:-1] != t.shape[:-1]:
            raise ValueError(f"DNeRFNGP.{who}: needs xyz [..., 3] and t [..., 1] with the same leading shape")
        if xyz.dtype != torch.float32 or t.dtype != torch.float32:
            raise NotImplementedError(f"DNeRFNGP.{who}: fp32 only (got {xyz.dtype}, {t.dtype})")
        if xyz.requires_grad or t.requires_grad:
            raise NotImplementedError(f"DNeRFNGP.{who}: the gradients with respect to the positions and the frame numbers are not "
                                      "built; inputs that require grad are refused")
        self._check_tables()
        if not xyz.is_cuda or not t.is_cuda:
            raise _lib.NerfLibraryError(f"DNeRFNGP.{who} needs tensors on a GPU (cuda) device; got a CPU tensor (there is no CPU fallback)")

    def compute_delta(self, xyz, t):
        """xyz [..., 3] in [0, 1], t [..., 1] frame numbers -> delta [..., 3], the field's value (at frame 0 too)."""
        self._check_inputs(xyz, t, "compute_delta")
        x, time = xyz.reshape(-1, 3).contiguous(), t.reshape(-1).contiguous()
        if x.shape[0] == 0:
            return xyz.new_zeros(xyz.shape)
        return self._apply_field(x, time, None, x.shape[0], x.shape[0], 1, "delta").view(xyz.shape)

    def forward(self, x, wbounds=None):
        """x [..., 4]: world position and, in the last column, the frame number of the point -> the encoding [..., out_dim]."""
        if not isinstance(x, torch.Tensor) or x.shape[-1:] != (4,):
            raise ValueError("DNeRFNGP.forward: x must be [..., 4] (xyz and the frame number)")
        xyz, t = x[..., :3], x[..., 3:]
        self._check_inputs(xyz, t, "forward")
        inputs = normalize_to_bounds(xyz, wbounds).reshape(-1, 3).contiguous()
        enc = self.encoder
        if inputs.shape[0] == 0:
            return x.new_zeros(list(x.shape[:-1]) + [self.out_dim])
        warped = self.warp(inputs, t.reshape(-1).contiguous())
        out = hash_encode(warped, enc.embeddings, enc.offsets, enc.per_level_scale, enc.base_resolution, enc.deterministic)
        return out.view(list(x.shape[:-1]) + [self.out_dim])

    def compute_tv_loss(self, xyz, t, wbounds):
        """The reference's smoothness term, [B, 1]: with the batch at frame 0 (its first point decides, as in the reference) the
        squared offset itself, otherwise the squared difference of the offsets at t and t - 1, summed over points and axes.  A loss,
        not the render path: the powers and sums are torch operations."""
        if xyz.dim() != 3 or t.dim() != 3:
            raise ValueError("DNeRFNGP.compute_tv_loss: needs xyz [B, N, 3] and t [B, N, 1]")
        self._check_inputs(xyz, t, "compute_tv_loss")
        inputs = normalize_to_bounds(xyz, wbounds)
        if t[0, 0].item() == 0.0:
            delta = self.compute_delta(inputs, t)
        else:
            delta = self.compute_delta(inputs, t) - self.compute_delta(inputs, t - 1.0)
        return delta.pow(2).sum(dim=1).sum(dim=1, keepdim=True)
