"""Hash-grid radiance field (instant-NGP style) on the kernels this package already has, and its renderer.

    HashField(bbox, encoder=None, geo_dim=16, width=64, sigma_hidden=1, color_hidden=2)      nn.Module
        sigma, geo = sigma_net(encoder(x)),  rgb = color_net(geo, SH4(view direction));  density(xyz), occupancy_grid(N, level, dilate),
        density_gradient(xyz), vertex_normals(vertices), vertex_colors(vertices, viewdirs)
    HashRenderer(field)            Renderer's call surface: render(batch) -> (rgb [B*N,3], depth [B*N]); render_geometry(batch) -> (rgb,
                                   depth, acc, normal); ray_gradients = True: rays that require grad get their gradient

The encoder runs on hash_encode, the two networks on fused_mlp, the grid lookup on nerf_occupancy_mark / nerf_compact_valid and the
image on nerf_composite, all as they are; what lies between them on the ray side (sample positions, the SH basis, the colour
network's input rows, the scatter into `raw`) are the HIP kernels of csrc/nerf_hashfield.hip.inc (include/nerf_mi355x_nn.h has every
formula).  The spatial adjoint of that glue -- the density gradient, the geometry outputs, gradients with respect to the rays --
is DESIGN.md section 2.14.1, its formulas in include/nerf_mi355x_field.h.  Where the samples of a ray lie -- one shared table, or
depths resampled from the field's own density (HashRenderer.N_importance) with stratified jitter (HashRenderer.perturb) -- is
DESIGN.md section 2.14.2, include/nerf_mi355x_sampling.h; the random draws of perturb are torch.rand.  No other ATen op computes on the render path: torch allocates,
zero-fills and slices.  fp32 only; CPU tensors raise NerfLibraryError: there is no eager fallback.

A DYNAMIC field is HashField(bbox, encoder=DNeRFNGP(num_frames, ...)) (deform.py): the normalised positions
are warped by the frame number of their ray (batch["time"]: [B], [B,1] or [B,N]) in one more launch, nerf_deform_forward, between
nerf_field_points and hash_encode; field.num_frames is None for a static field, which runs the launches it always ran.
density(xyz, time=k) is frame k.  The spatial adjoint, the geometry outputs, occupancy grids and deterministic=True are refused for a
dynamic field.

One host synchronisation per chunk on the culled path (HashRenderer.occupancy set): the number of surviving samples is read back,
because hash_encode and fused_mlp take their row count from the host.  Without a grid nothing synchronises.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .fused_mlp import MAX_ROWS, FusedMLP, fused_mlp
from .deform import DNeRFNGP
from .hashgrid import EPS, HashEncoder, _as_offsets, _flag, hash_encode, level_scales

GEO_DIM = 16                        # columns of the geometry feature: what the glue kernels move
SH_DIM = 16                         # real spherical harmonics of degree 0..3
MAX_SAMPLES = 192                   # nerf_composite's limit
DENSITY_ROWS = 1 << 22              # rows of one launch chain in HashField.density
GRADIENT_ROWS = 1 << 20             # ... and in HashField.density_gradient, which keeps save, gsave, features and their gradient per row


def box_frame(wbounds):
    """(box_min, box_max, extent) of the normalisation, from 6 fp32 numbers: extent = fp32(float64(largest fp32 axis extent) + 1e-6),
    the divisor of hashgrid.normalize_to_bounds (the subtraction in fp32, the sum in float64, rounded once)."""
    w = np.asarray(wbounds, dtype=np.float32).reshape(6)
    lo, hi = w[:3], w[3:]
    extent = np.float32(np.float64((hi - lo).max()) + EPS)
    return lo, hi, extent


class _Points(torch.autograd.Function):
    """World points [n,3] -> their normalised positions x [n,3] (nerf_field_points in point mode); the backward is
    nerf_field_points_backward in point mode, the compact layout."""

    @staticmethod
    def forward(ctx, pts, frame):
        pts = pts.detach().contiguous()
        n = pts.shape[0]
        x = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
        _lib.call("nerf_field_points", pts, None, None, 0, n, 1, None, n, *frame, x)
        ctx.save_for_backward(pts)
        ctx.frame = frame
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x):
        pts, = ctx.saved_tensors
        n = pts.shape[0]
        g_p = torch.empty_like(pts)
        _lib.call("nerf_field_points_backward", pts, None, None, 0, n, 1, None, n, *ctx.frame, g_x.contiguous(), None, 0, g_p, None, None)
        return g_p, None


class _RayInputs(torch.autograd.Function):
    """(o, d) [n,3] -> (x [M,3], sh [n,16]): nerf_field_points and nerf_sh4_encode, the two launches of the plain path.  The backward
    takes (g_x, g_sh) and writes g_o and g_d once: nerf_sh4_encode_backward, then nerf_field_points_backward with its view term."""

    @staticmethod
    def forward(ctx, o, d, t, index, M, S, frame, stride=0):
        o, d = o.detach().contiguous(), d.detach().contiguous()
        n = o.shape[0]
        x = torch.empty(M, 3, dtype=torch.float32, device=o.device)
        _lib.call("nerf_field_points", o, d, t, stride, n, S, index, M, *frame, x)
        sh = torch.empty(n, SH_DIM, dtype=torch.float32, device=o.device)
        _lib.call("nerf_sh4_encode", d, n, sh)
        ctx.save_for_backward(o, d, t)
        ctx.index, ctx.M, ctx.S, ctx.frame, ctx.stride = index, M, S, frame, stride
        ctx.set_materialize_grads(False)
        return x, sh

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x, g_sh):
        o, d, t = ctx.saved_tensors
        n, M = o.shape[0], ctx.M
        g_view = None
        if g_sh is not None:
            g_view = torch.empty(n, 3, dtype=torch.float32, device=o.device)
            _lib.call("nerf_sh4_encode_backward", d, g_sh.contiguous(), n, g_view)
        g_x = torch.zeros(M, 3, dtype=torch.float32, device=o.device) if g_x is None else g_x.contiguous()
        g_o, g_d = torch.empty_like(o), torch.empty_like(d)
        _lib.call("nerf_field_points_backward", o, d, t, ctx.stride, n, ctx.S, ctx.index, M, *ctx.frame, g_x, g_view, 0, None, g_o, g_d)
        return g_o, g_d, None, None, None, None, None, None


class _ColorInputs(torch.autograd.Function):
    """geo [M,16], sh [n,16] -> (cin [M,32], sigma_rows [M]); the backward writes g_geo from both incoming gradients and, when sh
    needs one (HashRenderer.ray_gradients), g_sh [n,16] by nerf_field_sh_gradient."""

    @staticmethod
    def forward(ctx, geo, sh, index, M, n, S):
        geo = geo.detach().contiguous()
        cin = torch.empty(M, GEO_DIM + SH_DIM, dtype=torch.float32, device=geo.device)
        sigma_rows = torch.empty(M, dtype=torch.float32, device=geo.device)
        _lib.call("nerf_field_color_inputs", geo, sh, index, M, n, S, cin, sigma_rows)
        ctx.M, ctx.index, ctx.n, ctx.S = M, index, n, S
        return cin, sigma_rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cin, g_sigma_rows):
        g_cin = g_cin.contiguous()
        g_geo = torch.empty(ctx.M, GEO_DIM, dtype=torch.float32, device=g_cin.device)
        _lib.call("nerf_field_color_inputs_backward", g_cin, g_sigma_rows.contiguous(), ctx.M, g_geo)
        g_sh = None
        if ctx.needs_input_grad[1]:
            g_sh = torch.empty(ctx.n, SH_DIM, dtype=torch.float32, device=g_cin.device)
            _lib.call("nerf_field_sh_gradient", g_cin, ctx.index, ctx.M, ctx.n, ctx.S, g_sh)
        return g_geo, g_sh, None, None, None, None


class _RawScatter(torch.autograd.Function):
    """rgb [M,3], sigma_rows [M] -> raw [n,S,4], zero at the points the list leaves out; the backward is the gather."""

    @staticmethod
    def forward(ctx, rgb, sigma_rows, index, M, n, S):
        raw = torch.zeros(n, S, 4, dtype=torch.float32, device=rgb.device)
        _lib.call("nerf_field_raw_scatter", rgb.detach().contiguous(), sigma_rows.detach().contiguous(), index, M, n * S, raw)
        ctx.index, ctx.M = index, M
        return raw

    @staticmethod
    @once_differentiable
    def backward(ctx, g_raw):
        g_raw = g_raw.contiguous()
        g_rgb = torch.empty(ctx.M, 3, dtype=torch.float32, device=g_raw.device)
        g_sigma_rows = torch.empty(ctx.M, dtype=torch.float32, device=g_raw.device)
        _lib.call("nerf_field_raw_gather", g_raw, ctx.index, ctx.M, g_raw.numel() // 4, g_rgb, g_sigma_rows)
        return g_rgb, g_sigma_rows, None, None, None, None


class _Composite(torch.autograd.Function):
    """raw [n,S,4] -> (rgb [n,3], depth [n]) by nerf_composite; the backward is nerf_composite_backward with g_t = NULL (the depths
    are constants, also where they are a table per ray: stride = S)."""

    @staticmethod
    def forward(ctx, raw, tvals, white, stride=0):
        raw = raw.detach()
        n, S = raw.shape[0], raw.shape[1]
        rgb = torch.empty(n, 3, dtype=torch.float32, device=raw.device)
        depth = torch.empty(n, dtype=torch.float32, device=raw.device)
        _lib.call("nerf_composite", raw, tvals, stride, n, S, white, rgb, depth, None)
        ctx.save_for_backward(raw, tvals)
        ctx.white, ctx.stride = white, stride
        ctx.set_materialize_grads(False)
        return rgb, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rgb, g_depth):
        raw, tvals = ctx.saved_tensors
        n, S = raw.shape[0], raw.shape[1]
        g_rgb = torch.zeros(n, 3, dtype=torch.float32, device=raw.device) if g_rgb is None else g_rgb.contiguous()
        g_depth = None if g_depth is None else g_depth.contiguous()
        g_raw = torch.empty_like(raw)
        _lib.call("nerf_composite_backward", raw, tvals, ctx.stride, n, S, ctx.white, g_rgb, g_depth, g_raw, None)
        return g_raw, None, None, None


class HashField(nn.Module):
    """x in `bbox` -> hash encoding -> sigma_net -> 16 columns: column 0 is the raw (pre-ReLU) density, all 16 are the geometry
    feature; (geometry feature, 16 SH coefficients of the view direction) -> color_net -> the pre-sigmoid rgb.

    bbox: 6 numbers, min xyz then max xyz; kept as the persistent fp32 buffer `wbounds`, so a checkpoint carries it.  encoder: a 3-D
    HashEncoder (default: L=16, C=2, H=16, T=19, desired_resolution=2048: 32 channels).  State-dict keys: encoder.embeddings,
    sigma_net.layers.{i}.{weight,bias}, color_net.layers.{i}.{weight,bias}, wbounds -- 11 parameter tensors with the defaults, one
    FusedAdam group.  deterministic=True sets the flag on both networks (FusedMLP.deterministic: exact, order-independent weight and
    bias gradients) and on the encoder when it is built here; an encoder that is passed in keeps its own.  With all three a training
    step is the same bytes from run to run."""

    def __init__(self, bbox, encoder=None, geo_dim=GEO_DIM, width=64, sigma_hidden=1, color_hidden=2, deterministic=False):
        super().__init__()
        _flag(deterministic, "HashField")
        if geo_dim != GEO_DIM:
            raise ValueError(f"HashField: geo_dim = {GEO_DIM} is built (the glue kernels move 16-column rows), got {geo_dim!r}")
        try:
            b = np.asarray(bbox, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"bbox must hold 6 numbers (min xyz, max xyz), got {bbox!r}") from None
        if b.shape != (6,) or not np.isfinite(b).all() or (b[3:] <= b[:3]).any():
            raise ValueError(f"bbox must hold 6 finite numbers (min xyz, max xyz) with a positive extent on every axis, got {bbox!r}")
        if encoder is None:
            encoder = HashEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                  desired_resolution=2048, deterministic=deterministic)
        if not isinstance(encoder, (HashEncoder, DNeRFNGP)) or encoder.input_dim != 3:
            raise TypeError("HashField: encoder must be a HashEncoder with input_dim = 3, or a DNeRFNGP")
        if isinstance(encoder, DNeRFNGP) and deterministic:
            raise NotImplementedError("HashField(deterministic=True) is not built for a dynamic field: the deformation tables' "
                                      "gradient is summed by atomics, so the promise of identical bytes would be false")
        self.encoder = encoder
        self.sigma_net = FusedMLP(encoder.out_dim, GEO_DIM, width, sigma_hidden, deterministic=deterministic)
        self.color_net = FusedMLP(GEO_DIM + SH_DIM, 3, width, color_hidden, deterministic=deterministic)
        # Compositing takes relu(sigma): a field whose density starts negative everywhere renders the background, has a gradient of
        # exactly zero and never trains.  With embeddings near zero the initial density is one constant of random sign, so the bias
        # of the density column starts at 1 -- a uniform fog, whose gradient reaches every parameter.
        with torch.no_grad():
            self.sigma_net.layers[-1].bias[0] = 1.0
        self.register_buffer("wbounds", torch.tensor(b, dtype=torch.float32), persistent=True)
        self._frame = None

    def frame(self):
        """(box_min, box_max, extent) as the HOST arguments of nerf_field_points, re-read from `wbounds` when it was written (a
        loaded checkpoint: one copy to the host)."""
        key = (self.wbounds.data_ptr(), self.wbounds._version)
        if self._frame is None or self._frame[0] != key:
            lo, hi, extent = box_frame(self.wbounds.detach().cpu().numpy())
            self._frame = (key, tuple(lo.tolist()), tuple(hi.tolist()), float(extent))
        return self._frame[1:]

    @property
    def bbox(self):
        """The box as 6 float64 numbers: the fp32 values of `wbounds`."""
        lo, hi, _ = self.frame()
        return np.array(list(lo) + list(hi), dtype=np.float64)

    @property
    def num_frames(self):
        """None for a static field; the frames of the deformation tables for a dynamic one (encoder = DNeRFNGP)."""
        return self.encoder.num_frames if isinstance(self.encoder, DNeRFNGP) else None

    def _static_only(self, what):
        if self.num_frames is not None:
            raise NotImplementedError(f"{what} is not built for a dynamic field (encoder = DNeRFNGP): the gradient of the warp "
                                      "with respect to the position, and a grid per frame, are not built")

    def _geo(self, x):
        """x [M,3] in [0,1] (a dynamic field: already warped) -> the 16 columns of sigma_net."""
        enc = self.encoder.encoder if isinstance(self.encoder, DNeRFNGP) else self.encoder
        feats = hash_encode(x, enc.embeddings, enc.offsets, enc.per_level_scale, enc.base_resolution, enc.deterministic)
        return fused_mlp(feats, [l.weight for l in self.sigma_net.layers], [l.bias for l in self.sigma_net.layers],
                         deterministic=self.sigma_net.deterministic)

    def _rgb(self, cin):
        return fused_mlp(cin, [l.weight for l in self.color_net.layers], [l.bias for l in self.color_net.layers],
                         deterministic=self.color_net.deterministic)

    def _check_fp32(self):
        for name, p in self.named_parameters():
            if p.dtype != torch.float32:
                raise NotImplementedError(f"HashField: fp32 only (parameter {name} is {p.dtype})")

    def _check_points(self, xyz, what):
        """The refusals of the entries that take world points, before any launch -> xyz, contiguous."""
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError(f"HashField.{what}: xyz must be a tensor [n, 3]")
        if xyz.dtype != torch.float32:
            raise NotImplementedError(f"HashField.{what}: fp32 only (xyz is {xyz.dtype})")
        self._check_fp32()
        if not xyz.is_cuda:
            raise _lib.NerfLibraryError(f"HashField.{what} needs xyz on a GPU (cuda) device; got a CPU tensor (there is no CPU fallback)")
        return xyz.contiguous()

    def density(self, xyz, time=None):
        """World points xyz [n,3] on the GPU -> the raw density [n,1]: the queryfn protocol of extract_mesh.  The positions are
        normalised by nerf_field_points in point mode; the parameters get gradients if they require them, and so does xyz (the
        point-mode adjoint nerf_field_points_backward behind the encoder's and the network's input gradients).
        time: a dynamic field needs it, ONE frame number (a float) for all points: extract_mesh(lambda p: field.density(p, time=k),
        ...) meshes frame k; its xyz must not require grad.  A static field takes no time."""
        dynamic = self.num_frames is not None
        if dynamic != (time is not None):
            raise ValueError("HashField.density: a dynamic field needs time (one frame number), a static field takes none")
        if dynamic and (isinstance(time, bool) or not isinstance(time, (int, float))):
            raise ValueError(f"HashField.density: time must be one number, got {time!r}")
        if dynamic and isinstance(xyz, torch.Tensor) and xyz.requires_grad:
            raise NotImplementedError("HashField.density: the gradient of the warp with respect to the position is not built; xyz "
                                      "that requires grad is refused for a dynamic field")
        xyz = self._check_points(xyz, "density")
        if xyz.shape[0] == 0:
            return xyz.new_zeros(0, 1)
        frame = self.frame()
        with_grad = xyz.requires_grad and torch.is_grad_enabled()
        if dynamic:                                   # one "ray" holds every point of a launch chain: n_samples = 1 and n "rays"
            frame_number = torch.full((min(xyz.shape[0], DENSITY_ROWS),), float(time), dtype=torch.float32, device=xyz.device)
        outs = []
        for i in range(0, xyz.shape[0], DENSITY_ROWS):
            pts = xyz[i:i + DENSITY_ROWS]
            n = pts.shape[0]
            if with_grad:
                x = _Points.apply(pts, frame)
            else:
                x = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
                _lib.call("nerf_field_points", pts, None, None, 0, n, 1, None, n, *frame, x)
            if dynamic:
                x = self.encoder.warp(x, frame_number[:n])
            outs.append(self._geo(x)[:, :1].contiguous())       # a copy of one column: the [n,16] output is not kept alive
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def _levels(self):
        """(offsets, scales, L): the level tables as the host arrays nerf_hashgrid_* take (what hash_encode builds per call)."""
        enc = self.encoder.encoder if isinstance(self.encoder, DNeRFNGP) else self.encoder
        offsets = _as_offsets(enc.offsets)
        L = offsets.shape[0] - 1
        scales = level_scales(L, enc.per_level_scale, enc.base_resolution)
        return (ctypes.c_int32 * (L + 1))(*offsets.tolist()), (ctypes.c_float * L)(*scales.tolist()), L

    def _sigma_gradient(self, x, positive_only):
        """x [M,3] in [0,1] -> (geo [M,16], g_x [M,3]): the density network's output and the gradient of its column 0, the raw
        density, with respect to x.  The launch chain of DESIGN.md section 2.14.1: nerf_hashgrid_forward, nerf_fused_mlp_forward with
        `save`, nerf_field_density_seed, nerf_fused_mlp_backward (no parameter gradient, grad_x given), nerf_hashgrid_backward
        (grad_emb = NULL).  Nothing is differentiated by autograd; M <= fused_mlp.MAX_ROWS."""
        enc, net, dev, M = self.encoder, self.sigma_net, x.device, x.shape[0]
        emb = enc.embeddings.detach().contiguous()
        offsets, scales, L = self._levels()
        C = emb.shape[1]
        weights = [l.weight.detach().contiguous() for l in net.layers]
        biases = [l.bias.detach().contiguous() for l in net.layers]
        none = [None] * len(weights)

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        feats = new(M, L * C)
        _lib.call("nerf_hashgrid_forward", x, emb, M, 3, C, L, offsets, scales, feats)
        geo = new(M, GEO_DIM)
        save = new(int(_lib.call("nerf_fused_mlp_save_floats", M, net.width, net.n_hidden)))
        _lib.call("nerf_fused_mlp_forward", feats, M, L * C, net.width, net.n_hidden, GEO_DIM, 0, weights, biases, geo, save)
        seed = new(M, GEO_DIM)
        _lib.call("nerf_field_density_seed", geo, GEO_DIM, M, int(bool(positive_only)), seed)
        gsave = new(int(_lib.call("nerf_fused_mlp_grad_floats", M, net.width, net.n_hidden, GEO_DIM)))
        g_feats = new(M, L * C)
        _lib.call("nerf_fused_mlp_backward", feats, None, seed, M, L * C, net.width, net.n_hidden, GEO_DIM, 0, weights, save, gsave,
                  none, none, g_feats)
        g_x = new(M, 3)
        _lib.call("nerf_hashgrid_backward", x, emb, g_feats, M, 3, C, L, offsets, scales, None, g_x)
        return geo, g_x

    def density_gradient(self, xyz, positive_only=False):
        """(sigma [n], grad [n,3]) at world points xyz [n,3] on the GPU: the raw density, bit-equal to density(xyz)[:, 0], and its
        gradient with respect to the world position (exactly zero on an axis along which the point lies outside the box: the
        normalisation clamps).  positive_only: grad is exactly zero wherever sigma <= 0.  Detached; no ATen op computes: the chain of
        _sigma_gradient between nerf_field_points and nerf_field_points_backward in point mode, in chunks of GRADIENT_ROWS points."""
        self._static_only("HashField.density_gradient")
        xyz = self._check_points(xyz, "density_gradient").detach()
        n_all = xyz.shape[0]
        sigma = torch.empty(n_all, dtype=torch.float32, device=xyz.device)
        grad = torch.empty(n_all, 3, dtype=torch.float32, device=xyz.device)
        frame = self.frame()
        for i in range(0, n_all, GRADIENT_ROWS):
            pts = xyz[i:i + GRADIENT_ROWS]
            n = pts.shape[0]
            x = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
            _lib.call("nerf_field_points", pts, None, None, 0, n, 1, None, n, *frame, x)
            geo, g_x = self._sigma_gradient(x, positive_only)
            _lib.call("nerf_field_points_backward", pts, None, None, 0, n, 1, None, n, *frame, g_x, None, 0, grad[i:i + n], None, None)
            sigma[i:i + n].copy_(geo[:, 0])                      # a copy of one column
        return sigma, grad

    def vertex_normals(self, vertices):
        """Unit outward normals [V,3] of an iso-surface of the density at its vertices [V,3]: -grad sigma / |grad sigma|, the zero
        vector where the gradient is zero or not finite -- mesh.vertex_normals' semantics on density_gradient (every point, whatever
        the sign of sigma); the normalisation of the [V,3] result is three torch operations."""
        self._static_only("HashField.vertex_normals")
        _, g = self.density_gradient(self._as_points(vertices, "vertex_normals"), positive_only=False)
        nrm = g.norm(dim=-1, keepdim=True)
        ok = torch.isfinite(nrm) & (nrm > 0)
        return torch.where(ok, -g / torch.where(ok, nrm, torch.ones_like(nrm)), torch.zeros_like(g))

    def vertex_colors(self, vertices, viewdirs=None):
        """Colours [V,3] fp32 in [0,1] at the vertices [V,3]: the sigmoid of the colour network's output for the view directions
        `viewdirs` [V,3] (direction of travel; None: every vertex seen head-on from outside, -vertex_normals, (0, 0, 1) where the
        normal is zero) -- mesh.vertex_colors' semantics.  The rows go through nerf_field_points (point mode), nerf_sh4_encode and
        nerf_field_color_inputs with n_samples = 1; the sigmoid of the [V,3] result is one torch operation."""
        from .mesh import _head_on
        self._static_only("HashField.vertex_colors")
        if isinstance(vertices, torch.Tensor) and viewdirs is not None and \
                (not isinstance(viewdirs, torch.Tensor) or viewdirs.shape != vertices.shape):
            raise ValueError(f"viewdirs must be a tensor of the vertices' shape {tuple(vertices.shape)}")
        pts = self._as_points(vertices, "vertex_colors")
        if pts.shape[0] == 0:
            return torch.empty(0, 3, dtype=torch.float32, device=pts.device)
        if viewdirs is None:
            viewdirs = _head_on(self.vertex_normals(pts))
        dirs = viewdirs.detach().to(device=pts.device, dtype=torch.float32).contiguous()
        frame = self.frame()
        out = torch.empty(pts.shape[0], 3, dtype=torch.float32, device=pts.device)
        with torch.no_grad():
            for i in range(0, pts.shape[0], DENSITY_ROWS):
                p, d = pts[i:i + DENSITY_ROWS], dirs[i:i + DENSITY_ROWS]
                n = p.shape[0]
                x = torch.empty(n, 3, dtype=torch.float32, device=p.device)
                _lib.call("nerf_field_points", p, None, None, 0, n, 1, None, n, *frame, x)
                sh = torch.empty(n, SH_DIM, dtype=torch.float32, device=p.device)
                _lib.call("nerf_sh4_encode", d, n, sh)
                cin, _ = _ColorInputs.apply(self._geo(x), sh, None, n, n, 1)
                out[i:i + n] = torch.sigmoid(self._rgb(cin))
        return out

    def _as_points(self, vertices, what):
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError(f"HashField.{what}: vertices must be a tensor [V, 3]")
        return self._check_points(vertices.detach().to(torch.float32), what)

    def occupancy_grid(self, N=128, level=0.0, dilate=1):
        """OccupancyGrid.from_fields(bbox, fine=<the density on an N grid over the box>): where sigma can exceed `level` now.  Runs
        under no_grad, the grid in x-slabs.  The grid carries no staleness key: rebuild it on your own schedule while training."""
        from .mesh import _query_grid, grid_axes
        from .occupancy import OccupancyGrid
        self._static_only("HashField.occupancy_grid")
        bbox = self.bbox
        axes, _, _ = grid_axes(bbox, N)
        field = _query_grid(self.density, axes, self.wbounds.device)
        return OccupancyGrid.from_fields(bbox, fine=field, level=level, dilate=dilate)


class HashRenderer:
    """Renderer's call surface over a HashField: render(batch) -> (rgb [B*N,3], depth [B*N]) with batch["rays_o"], batch["rays_d"]
    [B,N,3] on the GPU.

    N_samples (192; any int in [1, 192]) depths per ray, one shared table linspace(t_near, t_far, N_samples).  N_importance (0; with
    Sf = N_importance > 0, N_samples = Sc >= 3 is the coarse count and Sc + Sf <= 192): a coarse pass under no_grad -- the density
    network alone on the Sc depths, nerf_composite's weights -- then nerf_field_sample_importance draws Sf more depths per ray from
    those weights (u = linspace(0, 1, Sf)), and the image is rendered on the Sc + Sf merged depths.  The merged depths are constants:
    no gradient reaches the coarse pass, the fine pass trains the one field.  perturb (False; True: the coarse depths are jittered
    inside their strata, nerf_field_stratified_depths, and u is random; both come from _rand, drawn once per render() for all rays,
    so torch.manual_seed controls the image and chunk_rays does not).  samples: None, or a list that receives (t_coarse,
    weights_coarse, t_merged) per chunk with N_importance > 0.
    white_bkgd (True).  occupancy: None, or an OccupancyGrid with a fine bitfield (HashField.occupancy_grid): the
    samples in empty cells are not evaluated and keep raw = 0 -- at the price of ONE HOST SYNCHRONISATION PER CHUNK, the count of the
    surviving samples.  stats: None, or a list that receives (evaluated, total) samples per chunk on the culled path.  chunk_rays
    (16384): rays per launch chain; the result does not depend on it.

    Under no_grad, or when no parameter requires grad, the result is detached.  Otherwise the same launches run through autograd
    functions and every parameter that requires grad gets its gradient.  ray_gradients (False): rays that require grad are refused;
    True: they get their gradients too -- the same forward launches inside one autograd function whose backward writes g_rays_o and
    g_rays_d once (nerf_sh4_encode_backward, nerf_field_points_backward), with or without a grid, with trainable or frozen parameters.
    render_geometry(batch) adds the accumulated opacity and the composited analytic normal; geometry_chunk_rays (4096) is its chunk.
    `net` is the field: training.train_step(renderer, optimizer, ...) works as with a Renderer."""

    def __init__(self, field):
        if not isinstance(field, HashField):
            raise TypeError("HashRenderer needs a HashField")
        self.field = field
        self.N_samples = MAX_SAMPLES
        self.N_importance = 0
        self.perturb = False
        self.samples = None
        self.t_near, self.t_far = 2.0, 6.0
        self.white_bkgd = True
        self.occupancy = None
        self.chunk_rays = 16384
        self.geometry_chunk_rays = 4096
        self.ray_gradients = False
        self.stats = None
        self._tables = {}
        self._u_table = None

    @property
    def net(self):
        return self.field

    def _get_table(self, dev):
        key = (dev, float(self.t_near), float(self.t_far), int(self.N_samples))
        t = self._tables.get(key)
        if t is None:
            self._tables.clear()
            t = self._tables[key] = torch.linspace(self.t_near, self.t_far, self.N_samples).to(dev)
        return t

    def _get_u(self, dev):
        """The u of the deterministic resampling, linspace(0, 1, N_importance), built on the CPU like the depth table."""
        key = (dev, int(self.N_importance))
        if self._u_table is None or self._u_table[0] != key:
            self._u_table = (key, torch.linspace(0.0, 1.0, self.N_importance).to(dev))
        return self._u_table[1]

    def _rand(self, shape, device):
        """The random draws of perturb = True (Renderer._rand's signature): torch.rand on the rays' device, so torch.manual_seed
        controls the samples.  Overridable: tests replay recorded draws through it."""
        return torch.rand(*shape, device=device)

    def _check(self, rays_o, rays_d, geometry=False, batch=None):
        """Everything that is refused, before any launch or allocation -> the grid or None.  batch: render()'s, whose "time" a
        dynamic field needs."""
        if self.field.num_frames is not None:
            if geometry:
                self.field._static_only("HashRenderer.render_geometry")
            if self.occupancy is not None:
                self.field._static_only("HashRenderer.occupancy")
            if isinstance(rays_o, torch.Tensor) and isinstance(rays_d, torch.Tensor) and (rays_o.requires_grad or rays_d.requires_grad):
                self.field._static_only("HashRenderer.ray_gradients (rays that require grad)")
        S = self.N_samples
        if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= MAX_SAMPLES:
            raise ValueError(f"HashRenderer.N_samples must be an int in [1, {MAX_SAMPLES}], got {S!r}")
        Sf = self.N_importance
        if isinstance(Sf, bool) or not isinstance(Sf, int) or not 0 <= Sf <= MAX_SAMPLES - S:
            raise ValueError(f"HashRenderer.N_importance must be an int in [0, {MAX_SAMPLES} - N_samples], got {Sf!r}")
        if Sf > 0 and S < 3:
            raise ValueError(f"HashRenderer.N_importance > 0 needs N_samples >= 3 coarse depths (one interior weight at least), got {S!r}")
        if not isinstance(self.perturb, bool):
            raise ValueError(f"HashRenderer.perturb must be a bool, got {self.perturb!r}")
        if geometry and self.perturb:
            raise NotImplementedError("HashRenderer.render_geometry: perturb = True is not supported (geometry is rendered on the "
                                      "deterministic depths)")
        S = S + Sf
        if isinstance(self.chunk_rays, bool) or not isinstance(self.chunk_rays, int) or self.chunk_rays < 1:
            raise ValueError(f"HashRenderer.chunk_rays must be an int >= 1 (rays), got {self.chunk_rays!r}")
        if not isinstance(self.ray_gradients, bool):
            raise ValueError(f"HashRenderer.ray_gradients must be a bool, got {self.ray_gradients!r}")
        if geometry:
            g = self.geometry_chunk_rays
            if isinstance(g, bool) or not isinstance(g, int) or not 1 <= g <= MAX_ROWS // S:
                raise ValueError(f"HashRenderer.geometry_chunk_rays must be an int in [1, {MAX_ROWS} // N_samples] (rays), got {g!r}")
        grid = self.occupancy
        if grid is not None:
            from .occupancy import OccupancyGrid
            if not isinstance(grid, OccupancyGrid):
                raise TypeError("HashRenderer.occupancy must be an OccupancyGrid or None")
            if grid.bits["fine"] is None:
                raise ValueError("HashRenderer.occupancy needs a grid with a fine bitfield")
        if rays_o.dim() != 3 or rays_o.shape[-1] != 3 or rays_d.shape != rays_o.shape:
            raise ValueError("HashRenderer.render: rays_o and rays_d must both be [B, N, 3]")
        if rays_o.requires_grad or rays_d.requires_grad:
            if geometry:
                raise NotImplementedError("HashRenderer.render_geometry: rays that require grad are not supported (inference only)")
            if not self.ray_gradients:
                raise NotImplementedError("HashRenderer: rays that require grad are not supported (the ray adjoint runs only with "
                                          "HashRenderer.ray_gradients = True)")
            if Sf > 0:
                raise NotImplementedError("HashRenderer: rays that require grad are not supported with N_importance > 0 (the ray "
                                          "adjoint through resampled depths is not built)")
        if batch is not None and self.field.num_frames is not None:
            self._check_time(batch, rays_o)
        self.field._check_fp32()
        if not rays_o.is_cuda or not rays_d.is_cuda:
            raise _lib.NerfLibraryError("HashRenderer needs rays on a GPU (cuda) device; got a CPU tensor (there is no CPU fallback)")
        if grid is not None and grid.device != rays_o.device:
            raise ValueError(f"the occupancy grid is on {grid.device}, the rays on {rays_o.device}")
        return grid

    def _survivors(self, o, d, t, S, grid, stride=0):
        """(index, M) of a chunk: the ascending list of the point ids in occupied cells and their number, (None, n * S) without a
        grid.  With a grid this is the chunk's host synchronisation, and `stats` gets its (evaluated, total)."""
        dev, n = o.device, o.shape[0]
        P = n * S
        if grid is None:
            return None, P
        valid = torch.empty(n, S, dtype=torch.uint8, device=dev)
        _lib.call("nerf_occupancy_mark", o, d, t, stride, n, S, grid.bits["fine"], *grid.lookup_args(), 0, valid)
        index = torch.empty(P, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib.call("nerf_compact_valid_workspace_bytes", P)), dtype=torch.uint8, device=dev)
        _lib.call("nerf_compact_valid", valid, P, index, count, ws)
        M = int(count.item())                          # the host synchronisation of the culled path
        if isinstance(self.stats, list):
            self.stats.append((M, P))
        return index, M

    def _check_time(self, batch, rays_o):
        """batch["time"] of a dynamic field: frame numbers [B], [B,1] or [B,N], fp32, on the rays' device -> that tensor."""
        time = batch.get("time") if hasattr(batch, "get") else None
        B, N = rays_o.shape[0], rays_o.shape[1]
        if not isinstance(time, torch.Tensor):
            raise ValueError('HashRenderer.render: a dynamic field needs batch["time"], a tensor of frame numbers [B], [B,1] or [B,N]')
        if time.dtype != torch.float32 or time.device != rays_o.device:
            raise ValueError(f'HashRenderer.render: batch["time"] must be float32 on the rays\' device {rays_o.device}, got '
                             f"{time.dtype} on {time.device}")
        if tuple(time.shape) not in ((B,), (B, 1), (B, N)):
            raise ValueError(f'HashRenderer.render: batch["time"] must be [B], [B,1] or [B,N] = [{B}], [{B},1] or [{B},{N}], got '
                             f"{tuple(time.shape)}")
        if time.requires_grad:
            raise NotImplementedError("HashRenderer.render: the gradient with respect to the frame numbers is not built")
        return time

    def _time(self, batch, rays_o):
        """The frame number per ray [B*N] of a dynamic field, expanded from batch["time"] (validated by _check) without a
        synchronisation; None for a static field, which ignores the key."""
        if self.field.num_frames is None:
            return None
        B, N = rays_o.shape[0], rays_o.shape[1]
        return batch["time"].detach().reshape(B, -1).expand(B, N).reshape(-1).contiguous()

    def _chunk(self, o, d, t, S, grid, white, stride=0, time=None):
        """One chunk of n rays -> (rgb [n,3], depth [n]); every step is enqueued on the current stream.  t: the shared table [S]
        (stride 0) or the chunk's own depths [n,S] (stride S).  time [n] (a dynamic field): the positions are warped
        (nerf_deform_forward) between nerf_field_points and the encoder."""
        field, dev, n = self.field, o.device, o.shape[0]
        index, M = self._survivors(o.detach(), d.detach(), t, S, grid, stride)
        if M == 0:
            raw = torch.zeros(n, S, 4, dtype=torch.float32, device=dev)
        else:
            if torch.is_grad_enabled() and (o.requires_grad or d.requires_grad):       # (only with ray_gradients: _check)
                x, sh = _RayInputs.apply(o, d, t, index, M, S, field.frame(), stride)
            else:
                lo, hi, extent = field.frame()
                x = torch.empty(M, 3, dtype=torch.float32, device=dev)
                _lib.call("nerf_field_points", o, d, t, stride, n, S, index, M, lo, hi, extent, x)
                sh = torch.empty(n, SH_DIM, dtype=torch.float32, device=dev)
                _lib.call("nerf_sh4_encode", d, n, sh)
            if time is not None:
                x = field.encoder.warp(x, time, index, n, S)
            geo = field._geo(x)
            cin, sigma_rows = _ColorInputs.apply(geo, sh, index, M, n, S)
            raw = _RawScatter.apply(field._rgb(cin), sigma_rows, index, M, n, S)
        return _Composite.apply(raw, t, white, stride)

    def _draws(self, n, dev):
        """(jitter [n,Sc] or None, u, u's ray stride) of one render() call: with perturb the two _rand draws for ALL n rays, [n,Sc]
        first, then [n,Sf] only if Sf > 0 (the chunks take slices, so the image does not depend on chunk_rays); without, no jitter
        and the shared table linspace(0, 1, Sf).  u is None when N_importance is 0."""
        Sc, Sf = self.N_samples, self.N_importance
        if not self.perturb:
            return None, (self._get_u(dev) if Sf > 0 else None), 0
        jitter = self._rand((n, Sc), dev).to(torch.float32).contiguous()
        u = self._rand((n, Sf), dev).to(torch.float32).contiguous() if Sf > 0 else None
        return jitter, u, Sf

    def _depths(self, o, d, table, jitter, u, grid, white, time=None):
        """The depths one chunk of n rays is rendered on -> (t, S, ray stride), all constants (computed under no_grad).
        jitter [n,Sc] (or None): the coarse depths are nerf_field_stratified_depths of the table.  u (None: N_importance == 0) [Sf]
        or [n,Sf]: the coarse pass -- the survivors of the grid through nerf_field_points, hash_encode and sigma_net only, their
        densities scattered into a raw [n,Sc,4] (nerf_field_density_scatter), nerf_composite's weights -- and
        nerf_field_sample_importance, which gives the merged depths [n,Sc+Sf].  `samples` gets (t_coarse, weights, t_merged)."""
        field, dev, n = self.field, o.device, o.shape[0]
        Sc, Sf = self.N_samples, self.N_importance

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        with torch.no_grad():
            o, d = o.detach(), d.detach()
            t, stride = table, 0
            if jitter is not None:
                t, stride = new(n, Sc), Sc
                _lib.call("nerf_field_stratified_depths", table, jitter, n, Sc, t)
            if u is None:
                return t, Sc, stride
            index, M = self._survivors(o, d, t, Sc, grid, stride)
            raw = new(n, Sc, 4) if index is None else torch.zeros(n, Sc, 4, dtype=torch.float32, device=dev)
            if M > 0:
                x = new(M, 3)
                _lib.call("nerf_field_points", o, d, t, stride, n, Sc, index, M, *field.frame(), x)
                if time is not None:
                    x = field.encoder.warp(x, time, index, n, Sc)
                _lib.call("nerf_field_density_scatter", field._geo(x), GEO_DIM, index, M, n * Sc, raw)
            weights, rgb, depth = new(n, Sc), new(n, 3), new(n)
            _lib.call("nerf_composite", raw, t, stride, n, Sc, white, rgb, depth, weights)
            t_merged = new(n, Sc + Sf)
            _lib.call("nerf_field_sample_importance", weights, t, stride, u, 0 if u.dim() == 1 else Sf, n, Sc, Sf, t_merged, None)
        if isinstance(self.samples, list):
            self.samples.append((t, weights, t_merged))
        return t_merged, Sc + Sf, Sc + Sf

    def _geometry_chunk(self, o, d, t, S, grid, white, stride=0):
        """One chunk of n rays -> (rgb [n,3], depth [n], acc [n], normal [n,3]), detached: the launches of _chunk with the density
        network's `save` kept, then the gradient chain with positive_only on the surviving rows, scattered by id, and
        nerf_composite_normals."""
        field, dev, n = self.field, o.device, o.shape[0]

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        index, M = self._survivors(o, d, t, S, grid, stride)
        grad = new(n, S, 3)                            # rows of culled samples stay unwritten: their raw sigma is 0, they are not used
        if M == 0:
            raw = torch.zeros(n, S, 4, dtype=torch.float32, device=dev)
        else:
            frame = field.frame()
            x = new(M, 3)
            _lib.call("nerf_field_points", o, d, t, stride, n, S, index, M, *frame, x)
            geo, g_x = field._sigma_gradient(x, True)
            sh = new(n, SH_DIM)
            _lib.call("nerf_sh4_encode", d, n, sh)
            cin, sigma_rows = new(M, GEO_DIM + SH_DIM), new(M)
            _lib.call("nerf_field_color_inputs", geo, sh, index, M, n, S, cin, sigma_rows)
            raw = torch.zeros(n, S, 4, dtype=torch.float32, device=dev)
            _lib.call("nerf_field_raw_scatter", field._rgb(cin), sigma_rows, index, M, n * S, raw)
            _lib.call("nerf_field_points_backward", o, d, t, stride, n, S, index, M, *frame, g_x, None, 1, grad, None, None)
        rgb, depth, acc, normal = new(n, 3), new(n), new(n), new(n, 3)
        _lib.call("nerf_composite", raw, t, stride, n, S, white, rgb, depth, None)
        _lib.call("nerf_composite_normals", raw, t, stride, n, S, grad, normal, acc)
        return rgb, depth, acc, normal

    def render_geometry(self, batch):
        """(rgb [B*N,3], depth [B*N], acc [B*N], normal [B*N,3]): rgb and depth as render(batch) returns them (bit-equal), acc =
        sum_i w_i the accumulated opacity and normal = sum_i w_i n_i with n_i = -grad sigma / |grad sigma| at the samples with
        sigma_i > 0, else 0 (nerf_composite_normals; not renormalised, |normal| <= acc) -- Renderer.render_geometry's outputs.  The
        gradient is analytic, in world coordinates.  Honours occupancy and stats.  Inference only: rays
        that require grad are refused, the result is detached under any grad mode.  geometry_chunk_rays (4096) rays per launch
        chain (the chain keeps save, gsave, the features and their gradient per row); the result does not depend on it."""
        rays_o, rays_d = batch["rays_o"], batch["rays_d"]
        grid = self._check(rays_o, rays_d, geometry=True)
        dev = rays_o.device
        n = rays_o.shape[0] * rays_o.shape[1]

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if n == 0:
            return new(0, 3), new(0), new(0), new(0, 3)
        o = rays_o.reshape(-1, 3).to(torch.float32).contiguous()
        d = rays_d.reshape(-1, 3).to(torch.float32).contiguous()
        white, step = int(bool(self.white_bkgd)), self.geometry_chunk_rays
        table = self._get_table(dev)
        _, u, _ = self._draws(n, dev)                              # (perturb is refused: the shared u table, or None)
        outs = []
        with torch.no_grad():
            for i in range(0, n, step):
                oc, dc = o[i:i + step], d[i:i + step]
                t, S, stride = self._depths(oc, dc, table, None, u, grid, white)
                outs.append(self._geometry_chunk(oc, dc, t, S, grid, white, stride))
        if len(outs) == 1:
            return outs[0]
        return tuple(torch.cat([out[k] for out in outs], 0) for k in range(4))

    def render(self, batch):
        rays_o, rays_d = batch["rays_o"], batch["rays_d"]
        grid = self._check(rays_o, rays_d, batch=batch)
        tm = self._time(batch, rays_o)                             # None: a static field
        dev = rays_o.device
        n = rays_o.shape[0] * rays_o.shape[1]
        if n == 0:
            return torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
        o = rays_o.reshape(-1, 3).to(torch.float32).contiguous()
        d = rays_d.reshape(-1, 3).to(torch.float32).contiguous()
        S, white, step = self.N_samples, int(bool(self.white_bkgd)), self.chunk_rays
        t = self._get_table(dev)
        if self.N_importance == 0 and not self.perturb:            # the launches of a renderer without these attributes
            # time by keyword, and only for a dynamic field: a static field makes the calls it always made (tests replace
            # _chunk and _depths by functions with the static signature)
            outs = [self._chunk(o[i:i + step], d[i:i + step], t, S, grid, white, **({} if tm is None else {"time": tm[i:i + step]}))
                    for i in range(0, n, step)]
        else:
            jitter, u, u_stride = self._draws(n, dev)
            outs = []
            for i in range(0, n, step):
                oc, dc = o[i:i + step], d[i:i + step]
                extra = () if tm is None else (tm[i:i + step],)     # (a static field makes the calls it always made)
                tc, Sa, stride = self._depths(oc, dc, t, None if jitter is None else jitter[i:i + step],
                                              u[i:i + step] if u_stride else u, grid, white, *extra)
                outs.append(self._chunk(oc, dc, tc, Sa, grid, white, stride, *extra))
        if len(outs) == 1:
            return outs[0]
        return torch.cat([r for r, _ in outs], 0), torch.cat([z for _, z in outs], 0)
