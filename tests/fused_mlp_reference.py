"""float64 restatement of the fused MLP (include/nerf_mi355x_nn.h), written from its formulas: plain torch linear, ReLU and sigmoid
in float64 plus the analytic backward.  The yardstick of tests/test_gpu_fused_mlp.py and tests/test_gpu_image_fit.py; device-agnostic
(the tests run it on the GPU in float64), and it imports nothing of the package.

    h_0 = relu(W_0 x + b_0),  h_i = relu(W_i h_{i-1} + b_i),  z = W_out h_last + b_out,  y = z or sigmoid(z)

Every per-layer function takes the fp32 operands the kernel itself used (its own saved rows), so the checks built on them do not
compound and no ReLU decision can differ.  Each returns (truth, magnitude): the float64 value and the float64 sum of the absolute
values of the terms it was added up from, which is what a summation-order-free rounding bound scales with.
"""
import json
import os
import shutil

import torch

U = 2.0 ** -24
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(REPO, "profiles", "fused_mlp_parity.json")


def make_params(in_dim, width, n_hidden, out_dim, seed):
    """weights uniform in +-2/sqrt(fan_in), biases in +-0.5 (roughly half the units live on inputs in [0, 1)); CPU fp32 lists."""
    gen = torch.Generator().manual_seed(seed)
    weights, biases = [], []
    for i in range(n_hidden + 1):
        n_out, n_in = (out_dim if i == n_hidden else width), (width if i else in_dim)
        weights.append((torch.rand(n_out, n_in, generator=gen) * 2 - 1) * (2.0 / n_in ** 0.5))
        biases.append(torch.rand(n_out, generator=gen) - 0.5)
    return weights, biases


def make_inputs(B, in_dim, seed):
    return torch.rand(B, in_dim, generator=torch.Generator().manual_seed(seed))


def linear(inp, w, b):
    """pre-activation of one layer from fp32 operands -> (inp W^T + b, |inp| |W|^T + |b|), float64 [B, n_out]."""
    i64, w64, b64 = inp.double(), w.double(), b.double()
    return i64 @ w64.T + b64, i64.abs() @ w64.abs().T + b64.abs()


def forward(x, weights, biases, sigmoid):
    """The whole network in float64 -> (y, [h_0 .. h_last], [pre-activations of the hidden layers])."""
    h, hs, pres = x.double(), [], []
    for w, b in zip(weights[:-1], biases[:-1]):
        pre = h @ w.double().T + b.double()
        h = torch.relu(pre)
        pres.append(pre)
        hs.append(h)
    z = h @ weights[-1].double().T + biases[-1].double()
    return (torch.sigmoid(z) if sigmoid else z), hs, pres


def dz_out(grad_out, y, sigmoid):
    """dz of the output layer from fp32 grad_out and the forward's fp32 y."""
    g = grad_out.double()
    return g * y.double() * (1.0 - y.double()) if sigmoid else g


def transposed(dz_next, w_next):
    """W^T dz of one layer from fp32 operands -> (dz W, |dz| |W|), float64 [B, n_in]; the caller applies the ReLU mask."""
    d64, w64 = dz_next.double(), w_next.double()
    return d64 @ w64, d64.abs() @ w64.abs()


def weight_grad(dz, inp):
    """-> (dW, sum|term| of dW, db, sum|term| of db) of one layer from its fp32 dz [B, n_out] and input rows [B, n_in]."""
    d64, i64 = dz.double(), inp.double()
    return d64.T @ i64, d64.abs().T @ i64.abs(), d64.sum(0), d64.abs().sum(0)


def backward(x, weights, biases, grad_out, sigmoid):
    """The analytic backward of the whole network in float64 -> (grad_x, [grad_W], [grad_b])."""
    y, hs, _ = forward(x, weights, biases, sigmoid)
    dz = grad_out.double() * y * (1.0 - y) if sigmoid else grad_out.double()
    ins = [x.double()] + hs
    gw, gb = [None] * len(weights), [None] * len(weights)
    for i in range(len(weights) - 1, -1, -1):
        gw[i], gb[i] = dz.T @ ins[i], dz.sum(0)
        dz = dz @ weights[i].double()
        if i:
            dz = dz * (hs[i - 1] > 0)
    return dz, gw, gb


def parity_record(key, stats):
    """Keep the measured figures: merged into profiles/fused_mlp_parity.json.  Where NERF_PARITY_COPY_DIR names a directory (a run
    on a machine whose working tree does not come back), a copy of the file goes there as well."""
    rec = {}
    if os.path.exists(PARITY_JSON):
        with open(PARITY_JSON) as f:
            rec = json.load(f)
    rec[key] = stats
    os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
    with open(PARITY_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(PARITY_JSON, os.path.join(out, os.path.basename(PARITY_JSON)))
