"""Small fused ReLU MLP on the HIP kernels of csrc/nerf_fused_mlp.hip.inc (include/nerf_mi355x_nn.h).

    fused_mlp(x, weights, biases, output_activation=None, deterministic=False)   autograd function over nn.Linear-shaped lists
    FusedMLP(in_dim, out_dim, width=64, n_hidden=2, output_activation=None, deterministic=False)
    ImageFitNetwork(D=4, W=128, uv_encoder=None, chunk_size=16384, deterministic=False)
                                                               <- the reference's src/models/img_fit/network.py Network

One kernel runs the whole network, one more the gradient chain, and one weight-gradient launch per layer follows.  fp32 only (other
dtypes raise NotImplementedError); CPU tensors raise NerfLibraryError: there is no eager fallback.  The kernels read the parameter
tensors themselves at every call, so an in-place optimizer step is seen by the next call.  Double backward is not supported and raises.

deterministic=True sums the weight and bias gradients exactly in 64-bit fixed point (nerf_fused_mlp_backward_exact,
include/nerf_mi355x_nn_exact.h) instead of with fp32 atomics: the same bytes from run to run and under any
permutation of the rows.  The forward, the gradient chain and the input gradient are the same kernels either way.
"""
import sys
import types

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .hashgrid import _flag

WIDTHS = (64, 128)
MAX_IN_DIM = 256
MAX_HIDDEN = 8
MAX_OUT_DIM = 16
MAX_ROWS = 8388607                    # one call of the C entries (B * 256 < 2^31); larger batches run in chunks of this many rows
ACTIVATIONS = {None: 0, "none": 0, "sigmoid": 1}


def _check(x, weights, biases, output_activation):
    """Validate everything that can be wrong with the arguments, before the library is touched -> (in_dim, width, n_hidden, out_dim,
    activation code)."""
    if output_activation not in ACTIVATIONS:
        raise ValueError(f"fused_mlp: output_activation must be None or 'sigmoid' (got {output_activation!r})")
    weights, biases = list(weights), list(biases)
    if len(weights) != len(biases) or len(weights) < 2:
        raise ValueError("fused_mlp: weights and biases must list the hidden layers and the output layer (at least 2, equally many)")
    n_hidden = len(weights) - 1
    if n_hidden > MAX_HIDDEN:
        raise ValueError(f"fused_mlp: at most {MAX_HIDDEN} hidden layers are built (got {n_hidden})")
    if x.dim() < 1 or any(w.dim() != 2 for w in weights) or any(b.dim() != 1 for b in biases):
        raise ValueError("fused_mlp: x must be [..., in_dim], every weight [out, in] and every bias [out]")
    in_dim, width, out_dim = x.shape[-1], weights[0].shape[0], weights[-1].shape[0]
    if width not in WIDTHS:
        raise ValueError(f"fused_mlp: the hidden width must be one of {WIDTHS} (got {width})")
    if not 1 <= in_dim <= MAX_IN_DIM or not 1 <= out_dim <= MAX_OUT_DIM:
        raise ValueError(f"fused_mlp: 1 <= in_dim <= {MAX_IN_DIM} and 1 <= out_dim <= {MAX_OUT_DIM} are built (got {in_dim}, {out_dim})")
    for i, (w, b) in enumerate(zip(weights, biases)):
        want = (out_dim if i == n_hidden else width, width if i else in_dim)
        if tuple(w.shape) != want or tuple(b.shape) != want[:1]:
            raise ValueError(f"fused_mlp: layer {i} must have weight {list(want)} and bias {list(want[:1])} "
                             f"(got {list(w.shape)} and {list(b.shape)})")
    for t in [x] + weights + biases:
        if t.dtype != torch.float32:
            raise NotImplementedError(f"fused_mlp: fp32 only (got {t.dtype})")
    for t in [x] + weights + biases:
        if not t.is_cuda:
            raise _lib.NerfLibraryError("fused_mlp needs tensors on a GPU (cuda) device; got a CPU tensor (there is no CPU fallback)")
    return in_dim, width, n_hidden, out_dim, ACTIVATIONS[output_activation]


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, activation, n_layers, want_grad, deterministic, *params):
        # x [B, in_dim] (1 <= B <= MAX_ROWS), params = the weights then the biases; everything validated by fused_mlp().
        # deterministic: which entry sums the parameter gradients
        weights = [w.detach().contiguous() for w in params[:n_layers]]
        biases = [b.detach().contiguous() for b in params[n_layers:]]
        x = x.detach().contiguous()
        B, in_dim = x.shape
        width, n_hidden, out_dim = weights[0].shape[0], n_layers - 1, weights[-1].shape[0]
        out = torch.empty(B, out_dim, dtype=torch.float32, device=x.device)
        save = None
        if want_grad:                           # the SAVE forward only when something will be differentiated
            save = torch.empty(_lib.call("nerf_fused_mlp_save_floats", B, width, n_hidden), dtype=torch.float32, device=x.device)
        _lib.call("nerf_fused_mlp_forward", x, B, in_dim, width, n_hidden, out_dim, activation, weights, biases, out, save)
        if save is not None:
            ctx.save_for_backward(x, out, save, *weights)
            ctx.activation = activation
            ctx.deterministic = deterministic
        return out

    @staticmethod
    @once_differentiable                        # a double backward raises instead of returning zeros
    def backward(ctx, grad):
        x, out, save, *weights = ctx.saved_tensors
        n_layers = len(weights)
        B, in_dim = x.shape
        width, n_hidden, out_dim = weights[0].shape[0], n_layers - 1, weights[-1].shape[0]
        if grad.dtype != torch.float32:
            raise NotImplementedError(f"fused_mlp: fp32 only (the output gradient is {grad.dtype})")
        grad = grad.contiguous()
        need = ctx.needs_input_grad
        need_w, need_b = need[5:5 + n_layers], need[5 + n_layers:]
        # the entry accumulates into zeroed buffers
        grad_w = [torch.zeros_like(w) if need_w[i] else None for i, w in enumerate(weights)]
        grad_b = [torch.zeros(w.shape[0], dtype=torch.float32, device=x.device) if need_b[i] else None for i, w in enumerate(weights)]
        grad_x = torch.empty_like(x) if need[0] else None
        gsave = torch.empty(_lib.call("nerf_fused_mlp_grad_floats", B, width, n_hidden, out_dim), dtype=torch.float32, device=x.device)
        if ctx.deterministic and (any(need_w) or any(need_b)):
            nbytes = _lib.call("nerf_fused_mlp_exact_workspace_bytes", in_dim, width, n_hidden, out_dim)
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)      # the entry zero-fills it
            _lib.call("nerf_fused_mlp_backward_exact", x, out, grad, B, in_dim, width, n_hidden, out_dim, ctx.activation, weights, save,
                      gsave, grad_w, grad_b, grad_x, workspace, nbytes)
        else:
            _lib.call("nerf_fused_mlp_backward", x, out, grad, B, in_dim, width, n_hidden, out_dim, ctx.activation, weights, save, gsave,
                      grad_w, grad_b, grad_x)
        return (grad_x, None, None, None, None, *grad_w, *grad_b)


def fused_mlp(x, weights, biases, output_activation=None, deterministic=False):
    """x [..., in_dim] through relu(W_i . + b_i) for the hidden layers and act(W_out . + b_out) -> [..., out_dim].  `weights` and
    `biases` list the hidden layers in order, then the output layer, as nn.Linear holds them ([out, in] and [out]); the hidden width
    (64 or 128), the number of hidden layers (1..8) and out_dim (1..16) are inferred from the shapes.  output_activation: None or
    "sigmoid".  Gradients are computed for exactly those of x, weights and biases that require them (the one of x so that an
    encoder in front gets its own).
    deterministic=True: the gradients with respect to `weights` and `biases` are the exact, order-independent sums (the module's
    docstring).  A batch above MAX_ROWS still runs in chunks: each chunk's sum is exact, and autograd adds the chunks' gradients in
    fp32, in a fixed order -- reproducible from run to run, but no longer independent of how the rows fall into chunks."""
    _flag(deterministic, "fused_mlp")
    weights, biases = list(weights), list(biases)
    in_dim, width, n_hidden, out_dim, activation = _check(x, weights, biases, output_activation)
    prefix = list(x.shape[:-1])
    rows = x.reshape(-1, in_dim)
    if rows.shape[0] == 0:                       # nothing to run (the C entries refuse an empty batch)
        return x.new_zeros(prefix + [out_dim])
    # (Function.forward runs with grad mode off: whether anything will be differentiated is decided here)
    want_grad = torch.is_grad_enabled() and any(t.requires_grad for t in [x] + weights + biases)
    outs = [_FusedMLP.apply(rows[i:i + MAX_ROWS], activation, n_hidden + 1, want_grad, deterministic, *weights, *biases)
            for i in range(0, rows.shape[0], MAX_ROWS)]
    return (outs[0] if len(outs) == 1 else torch.cat(outs, 0)).view(prefix + [out_dim])


class FusedMLP(nn.Module):
    """in_dim -> n_hidden x (Linear(width) + ReLU) -> Linear(out_dim) [-> sigmoid], run by fused_mlp.  The parameters are plain
    nn.Linear modules with PyTorch's default init: state-dict keys layers.{i}.weight / layers.{i}.bias.  `deterministic` is a plain
    attribute, handed to fused_mlp at every call."""

    def __init__(self, in_dim, out_dim, width=64, n_hidden=2, output_activation=None, deterministic=False):
        super().__init__()
        if width not in WIDTHS or not 1 <= n_hidden <= MAX_HIDDEN or not 1 <= in_dim <= MAX_IN_DIM or not 1 <= out_dim <= MAX_OUT_DIM \
                or output_activation not in ACTIVATIONS:
            raise ValueError(f"FusedMLP: width in {WIDTHS}, 1 <= n_hidden <= {MAX_HIDDEN}, 1 <= in_dim <= {MAX_IN_DIM}, 1 <= out_dim <= "
                             f"{MAX_OUT_DIM} and output_activation None or 'sigmoid' are built (got {width}, {n_hidden}, {in_dim}, "
                             f"{out_dim}, {output_activation!r})")
        self.in_dim, self.out_dim, self.width, self.n_hidden = in_dim, out_dim, width, n_hidden
        self.output_activation = output_activation
        self.deterministic = _flag(deterministic, "FusedMLP")
        self.layers = nn.ModuleList([nn.Linear(in_dim, width)] + [nn.Linear(width, width) for _ in range(n_hidden - 1)] +
                                    [nn.Linear(width, out_dim)])

    def forward(self, x):
        return fused_mlp(x, [l.weight for l in self.layers], [l.bias for l in self.layers], self.output_activation, self.deterministic)


def frequency_encode(x, freq):
    """The reference's frequency encoding (src/models/encoding/freq.py with include_input and log sampling): the input, then sin and
    cos of x * 2^k for k = 0 .. freq-1 -> [..., input_dim * (1 + 2 * freq)]."""
    bands = 2.0 ** torch.linspace(0.0, freq - 1, steps=freq)
    return torch.cat([x] + [fn(x * band) for band in bands for fn in (torch.sin, torch.cos)], -1)


class _FrequencyEncoder:
    """Not an nn.Module, as in the reference: it has no parameters and adds no state-dict keys."""

    def __init__(self, input_dim=2, freq=10, **kwargs):
        self.input_dim, self.freq = input_dim, freq
        self.out_dim = input_dim * (1 + 2 * freq)

    def __call__(self, x):
        return frequency_encode(x, self.freq)


class ImageFitNetwork(nn.Module):
    """The reference's image-fit Network (src/models/img_fit/network.py) without its global cfg: uv -> encoding -> D x (Linear(W) +
    ReLU) -> Linear(3) + sigmoid.  Member names and state-dict keys are the reference's (backbone_layer.{i}, output_layer.0, and
    uv_encoder.embeddings with a hash grid); the layers run through fused_mlp, so W must be 64 or 128 and 1 <= D <= 8.

    uv_encoder is a dict in the reference's config vocabulary: {"type": "frequency", "input_dim": 2, "freq": 10} (the default, 42
    channels) or {"type": "cuda_hashgrid", ...HashEncoder's arguments}.  The frequency encoding is computed in eager torch: it is 42
    floats per pixel, and the C positional-encoding entry is 3-D only.  The hash grid is called with normalize=False: uv is already in
    [0, 1].  output_layer's nn.Sigmoid exists for key and structure parity and is not called: the kernel applies the sigmoid.
    deterministic (a plain attribute) is fused_mlp's flag; a hash-grid encoder keeps its own, given in the uv_encoder dict."""

    def __init__(self, D=4, W=128, uv_encoder=None, chunk_size=16384, deterministic=False):
        super().__init__()
        self.deterministic = _flag(deterministic, "ImageFitNetwork")
        enc = dict(uv_encoder) if uv_encoder is not None else {"type": "frequency", "input_dim": 2, "freq": 10}
        kind = enc.pop("type", None)
        if kind == "frequency":
            self.uv_encoder = _FrequencyEncoder(**enc)
        elif kind == "cuda_hashgrid":
            from .hashgrid import HashEncoder
            self.uv_encoder = HashEncoder(**enc)
        else:
            raise NotImplementedError(f"ImageFitNetwork: uv_encoder type {kind!r} is not built ('frequency' and 'cuda_hashgrid' are)")
        input_ch = self.uv_encoder.out_dim
        if W not in WIDTHS or not 1 <= D <= MAX_HIDDEN or not 1 <= input_ch <= MAX_IN_DIM:
            raise ValueError(f"ImageFitNetwork: W in {WIDTHS}, 1 <= D <= {MAX_HIDDEN} and at most {MAX_IN_DIM} encoding channels are "
                             f"built (got {W}, {D}, {input_ch})")
        self.chunk_size = int(chunk_size)
        self.backbone_layer = nn.ModuleList([nn.Linear(input_ch, W)] + [nn.Linear(W, W) for _ in range(D - 1)])
        self.output_layer = nn.Sequential(nn.Linear(W, 3), nn.Sigmoid())

    def render(self, uv, batch=None):
        layers = list(self.backbone_layer) + [self.output_layer[0]]
        encoding = self.uv_encoder(uv, normalize=False) if isinstance(self.uv_encoder, nn.Module) else self.uv_encoder(uv)
        rgb = fused_mlp(encoding, [l.weight for l in layers], [l.bias for l in layers], output_activation="sigmoid",
                        deterministic=self.deterministic)
        return {"rgb": rgb}

    def batchify(self, uv, batch):
        rets = [self.render(uv[i:i + self.chunk_size], batch) for i in range(0, max(uv.shape[0], 1), self.chunk_size)]
        return {k: torch.cat([r[k] for r in rets], dim=0) for k in rets[0]}

    def forward(self, batch):
        B, N_pixels, C = batch["uv"].shape
        ret = self.batchify(batch["uv"].reshape(-1, C), batch)
        return {k: ret[k].reshape(B, N_pixels, -1) for k in ret}


class _CallableModule(types.ModuleType):
    """The package exports the function under the name of this module, and importing a sub-module binds the MODULE to that name in
    the package: so the module itself is callable, and `nerf_replication_amd.fused_mlp(...)` works whichever of the two it finds."""

    def __call__(self, *args, **kwargs):
        return fused_mlp(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
