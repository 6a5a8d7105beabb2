"""GPU tests of the fused MLP's exact weight and bias gradients (csrc/nerf_fused_mlp_exact.hip.inc, include/nerf_mi355x_nn_exact.h,
DESIGN.md section 2.13.1) against the integer restatement in tests/fused_mlp_exact_reference.py.

What is asserted, and where the bounds come from:
  bits           every weight and bias gradient equals the restatement in every bit, computed from the kernel's own x, save and gsave,
                 into buffers pre-filled with non-zero values (and some -0.0): elements with emax = 0 keep their bits, the others are
                 fadd(previous, v).  The restatement sums integers, so there is one right answer.  Batches on both sides of the add
                 kernel's 1024 rows per workgroup and of its 32-row LDS chunk.
  singly         weights without bias, bias without weights, neither: what is not asked for keeps its bytes.
  same bytes     gsave and grad_x are nerf_fused_mlp_backward's; the gradients are the same from run to run and under permutations
                 of the rows.
  exactness      1 + 2^-30 - 1 into every element is exactly 2^-30, in every order of the rows.
  poison         one Inf in grad_out: quiet NaN where the restatement has it, the other elements as without it.
  accuracy       |got - truth| <= 2^-24 * sum|dz * in| + B * 2^(emax - 150 - K) + 2^-24 * |truth| per element (term formation,
                 truncation, the final rounding; DESIGN.md section 2.13.1 derives it): no tuned slack.  The worst ratios and the
                 accumulator's peak go to profiles/fused_mlp_exact_parity.json.
  module         fused_mlp, FusedMLP, ImageFitNetwork and HashField.density with the flag give the bytes of the direct call; 20
                 train_step calls of a HashField run twice give equal parameters and loss histories, with and without an occupancy
                 grid; one step's parameter gradients do not depend on the order of the rays.
Nothing is asserted with the flag off.  Every buffer the kernels write is the interior of a larger sentinel-filled one, the workspace
included."""
import json
import os
import shutil

import pytest
import torch

import fused_mlp_exact_reference as X
import fused_mlp_reference as R
import test_gpu_fused_mlp as G
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

#          in_dim width n_hidden out_dim sigmoid
CONFIGS = [(32, 64, 1, 16, False), (32, 64, 2, 3, False), (42, 128, 4, 3, True), (3, 64, 1, 1, False), (256, 128, 1, 16, False)]
_IDS = ["%dx%dx%d-%d%s" % (c[0], c[1], c[2], c[3], "-sigmoid" if c[4] else "") for c in CONFIGS]
ROWS_PER_WORKGROUP = 1024           # kFxRows of the add kernel (and kFxColRows of the column passes)
BATCHES = (1, 31, 33, 4113, ROWS_PER_WORKGROUP - 1, ROWS_PER_WORKGROUP, ROWS_PER_WORKGROUP + 1)
WIDEST_BATCHES = (1, 33, ROWS_PER_WORKGROUP, ROWS_PER_WORKGROUP + 1)      # 256 x 128: 35 000 terms per row on the CPU
WS_SENTINEL, WS_PAD = 0xA5, 256     # WS_PAD bytes on each side: the interior keeps the 16-byte alignment the entry asks for
PARITY_JSON = os.path.join(R.REPO, "profiles", "fused_mlp_exact_parity.json")
_worst = {}


CASES = [(cfg, B) for cfg in CONFIGS for B in (WIDEST_BATCHES if cfg[0] == 256 else BATCHES)]
_CASE_IDS = ["%s-B%d" % (_IDS[CONFIGS.index(cfg)], B) for cfg, B in CASES]


@pytest.fixture(scope="module", autouse=True)
def _keep_the_figures():
    """Writes the worst error / bound ratio per gradient kind and the accumulator's peak magnitude, as the tests of this module
    measured them, to profiles/fused_mlp_exact_parity.json (and a copy where NERF_PARITY_COPY_DIR names a directory)."""
    yield
    if _worst:
        os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
        with open(PARITY_JSON, "w") as f:
            json.dump({k: (round(v, 4) if isinstance(v, float) else v) for k, v in sorted(_worst.items())}, f, indent=1, sort_keys=True)
        out = os.environ.get("NERF_PARITY_COPY_DIR")
        if out:
            os.makedirs(out, exist_ok=True)
            shutil.copyfile(PARITY_JSON, os.path.join(out, os.path.basename(PARITY_JSON)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _workspace(amd, net):
    need = amd._lib.call("nerf_fused_mlp_exact_workspace_bytes", net.in_dim, net.width, net.n_hidden, net.out_dim)
    assert need == X.workspace_bytes(net.in_dim, net.width, net.n_hidden, net.out_dim)
    whole = torch.full((need + 2 * WS_PAD,), WS_SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[WS_PAD:WS_PAD + need], need


def _ws_intact(whole, need):
    return bool((whole[:WS_PAD] == WS_SENTINEL).all() and (whole[WS_PAD + need:] == WS_SENTINEL).all())


def _prefill(net, seed):
    """Non-zero previous contents of every gradient buffer (CPU), some of them -0.0."""
    gen = torch.Generator().manual_seed(seed)
    prev_w, prev_b = [], []
    for i in range(net.n_hidden + 1):
        n_out, n_in = net.layer_shape(i)
        w, b = torch.randn(n_out, n_in, generator=gen), torch.randn(n_out, generator=gen)
        w.view(-1)[::7] = -0.0
        b[::5] = -0.0
        prev_w.append(w)
        prev_b.append(b)
    return prev_w, prev_b


class Exact:
    """One nerf_fused_mlp_backward_exact call, every buffer inside sentinels.  want_w / want_b: the layers whose pointer is given
    (default all); prev: (weights, biases) the buffers hold before (default zeros)."""

    def __init__(self, amd, net, x, out, go, sv, sigmoid, prev=None, want_w=None, want_b=None, want_x=True):
        B, layers = x.shape[0], range(net.n_hidden + 1)
        self.gr = G.Grads(net, B, want_x=want_x)
        if prev is not None:
            for i in layers:
                self.gr.w[i][1].copy_(prev[0][i].reshape(-1))
                self.gr.b[i][1].copy_(prev[1][i].reshape(-1))
        gw = [self.gr.w[i][1] if want_w is None or i in want_w else None for i in layers]
        gb = [self.gr.b[i][1] if want_b is None or i in want_b else None for i in layers]
        ws_whole, ws, need = _workspace(amd, net)
        amd._lib.call("nerf_fused_mlp_backward_exact", x, out, go, *net.dims(B), int(sigmoid), net.w, sv, self.gr.gsave, gw, gb,
                      self.gr.gx if want_x else None, ws, need)
        torch.cuda.synchronize()
        assert G._intact(self.gr.whole_g, self.gr.n_gsave) and G._intact(self.gr.whole_x, B * net.in_dim) and _ws_intact(ws_whole, need)
        for i in layers:
            n_out, n_in = net.layer_shape(i)
            assert G._intact(self.gr.w[i][0], n_out * n_in) and G._intact(self.gr.b[i][0], n_out)
        self.w = [self.gr.w[i][1].view(net.layer_shape(i)) for i in layers]
        self.b = [self.gr.b[i][1] for i in layers]
        self.gsave, self.gx = self.gr.gsave, self.gr.gx


def _restate(net, B, x, sv, gsave, K, prev=None):
    """The restatement of every layer from the kernel's own operands -> ([weights], [biases]) result dicts."""
    ops = X.layer_operands(x.cpu().reshape(-1), sv.cpu().reshape(-1), gsave.cpu(), B, net.in_dim, net.width, net.n_hidden, net.out_dim)
    rw = [X.exact_weight_gradient(dz, inp, K, None if prev is None else prev[0][i]) for i, (dz, inp) in enumerate(ops)]
    rb = [X.exact_bias_gradient(dz, K, None if prev is None else prev[1][i]) for i, (dz, _) in enumerate(ops)]
    return rw, rb, ops


_cache = {}


def _case(amd, cfg, B):
    """Configuration cfg at batch B, computed once per module: the inputs, the forward, one exact backward into zeroed buffers and
    its restatement."""
    if (cfg, B) not in _cache:
        net = G.Net.get(cfg)
        x, go = G._inputs(net, B)
        out, sv = G._forward(amd, net, x, cfg[4])
        K = amd._lib.call("nerf_fused_mlp_exact_guard_bits", B)
        assert K == X.guard_bits(B)
        ex = Exact(amd, net, x, out, go, sv, cfg[4])
        rw, rb, ops = _restate(net, B, x, sv, ex.gsave, K)
        _cache[cfg, B] = dict(net=net, x=x, go=go, out=out, sv=sv, K=K, ex=ex, rw=rw, rb=rb, ops=ops)
    return _cache[cfg, B]


# ---- the direct call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B", CASES, ids=_CASE_IDS)
def test_bit_equal_to_the_restatement(amd, cfg, B):
    c = _case(amd, cfg, B)
    net = c["net"]
    differ = 0
    for i in range(net.n_hidden + 1):                                  # into zeroed buffers: the sums themselves
        differ += int((_bits(c["ex"].w[i].cpu()) != _bits(c["rw"][i]["grad"])).sum())
        differ += int((_bits(c["ex"].b[i].cpu()) != _bits(c["rb"][i]["grad"])).sum())
        assert c["rw"][i]["invariant"]
    print(f"    {_IDS[CONFIGS.index(cfg)]} B={B} K={c['K']}: {differ} elements differ")
    assert differ == 0
    prev = _prefill(net, B)
    ex = Exact(amd, net, c["x"], c["out"], c["go"], c["sv"], cfg[4], prev=([t.cuda() for t in prev[0]], [t.cuda() for t in prev[1]]))
    assert torch.equal(_bits(ex.gsave), _bits(c["ex"].gsave))
    touched = False
    for i in range(net.n_hidden + 1):
        for got, res, before in ((ex.w[i].cpu(), c["rw"][i], prev[0][i]), (ex.b[i].cpu(), c["rb"][i], prev[1][i])):
            want = X.finish(res["acc"], res["emax"], c["K"], before)
            assert torch.equal(_bits(got), _bits(want)), (B, i)
            idle = res["emax"] == 0
            assert torch.equal(_bits(got)[idle], _bits(before)[idle])   # not read, not written: -0.0 stays -0.0
            touched = touched or bool((got != before)[~idle].any())
    assert touched


def test_layers_asked_for_singly(amd):
    """Layer 0: the weights alone; layer 1: the bias alone; layer 2: neither."""
    cfg = CONFIGS[1]
    for B in (33, ROWS_PER_WORKGROUP + 1):
        c = _case(amd, cfg, B)
        net = c["net"]
        prev = _prefill(net, B + 1)
        ex = Exact(amd, net, c["x"], c["out"], c["go"], c["sv"], cfg[4], prev=([t.cuda() for t in prev[0]], [t.cuda() for t in prev[1]]),
                   want_w={0}, want_b={1})
        assert torch.equal(_bits(ex.w[0].cpu()), _bits(X.finish(c["rw"][0]["acc"], c["rw"][0]["emax"], c["K"], prev[0][0])))
        assert torch.equal(_bits(ex.b[1].cpu()), _bits(X.finish(c["rb"][1]["acc"], c["rb"][1]["emax"], c["K"], prev[1][1])))
        assert bool((ex.w[0].cpu() != prev[0][0]).any()) and bool((ex.b[1].cpu() != prev[1][1]).any())
        for got, before in ((ex.b[0], prev[1][0]), (ex.w[1], prev[0][1]), (ex.w[2], prev[0][2]), (ex.b[2], prev[1][2])):
            assert torch.equal(_bits(got.cpu()), _bits(before))             # the rest is untouched
        assert torch.equal(_bits(ex.gsave), _bits(c["ex"].gsave)) and torch.equal(_bits(ex.gx), _bits(c["ex"].gx))
        # nothing asked for at all, and no grad_x: the chain alone
        none = Exact(amd, net, c["x"], c["out"], c["go"], c["sv"], cfg[4], prev=([t.cuda() for t in prev[0]], [t.cuda() for t in prev[1]]),
                     want_w=set(), want_b=set(), want_x=False)
        assert torch.equal(_bits(none.gsave), _bits(c["ex"].gsave)) and bool((none.gx == G.SENTINEL).all())
        for i in range(3):
            assert torch.equal(_bits(none.w[i].cpu()), _bits(prev[0][i])) and torch.equal(_bits(none.b[i].cpu()), _bits(prev[1][i]))


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_same_bytes(amd, cfg):
    for B in (33, ROWS_PER_WORKGROUP + 1):
        c = _case(amd, cfg, B)
        net, first = c["net"], c["ex"]
        default = G.Grads(net, B)
        default.call(amd, c["x"], c["out"], c["go"], c["sv"], cfg[4])
        torch.cuda.synchronize()
        assert torch.equal(_bits(first.gsave), _bits(default.gsave)) and torch.equal(_bits(first.gx), _bits(default.gx))
        again = Exact(amd, net, c["x"], c["out"], c["go"], c["sv"], cfg[4])  # run to run
        for seed in (1, 2):
            perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed)).cuda()
            xp, gop = c["x"][perm].contiguous(), c["go"][perm].contiguous()
            outp, svp = G._forward(amd, net, xp, cfg[4])
            assert torch.equal(outp, c["out"][perm])                       # a row's result depends on that row alone
            moved = Exact(amd, net, xp, outp, gop, svp, cfg[4])
            for i in range(net.n_hidden + 1):
                assert torch.equal(_bits(moved.w[i]), _bits(first.w[i])) and torch.equal(_bits(moved.b[i]), _bits(first.b[i])), (B, seed, i)
        for i in range(net.n_hidden + 1):
            assert torch.equal(_bits(again.w[i]), _bits(first.w[i])) and torch.equal(_bits(again.b[i]), _bits(first.b[i]))
            assert float(first.w[i].abs().max()) > 0


class _Identity:
    """W_0 = I [64, 64], b_0 = 0, W_out = ones [1, 64], b_out = 0: with x = 1 every h is exactly 1 and dz_0 = grad_out in every column."""
    in_dim, width, n_hidden, out_dim = 64, 64, 1, 1

    def __init__(self):
        self.w = [torch.eye(64, device="cuda"), torch.ones(1, 64, device="cuda")]
        self.b = [torch.zeros(64, device="cuda"), torch.zeros(1, device="cuda")]

    def dims(self, B):
        return (B, 64, 64, 1, 1)

    def layer_shape(self, i):
        return (1, 64) if i else (64, 64)


def test_what_float_atomics_cannot_guarantee(amd):
    """Rows (1, 2^-30, -1) of grad_out: every element of every gradient is exactly 2^-30, in every order of the rows."""
    net = _Identity()
    assert amd._lib.call("nerf_fused_mlp_exact_guard_bits", 3) == 30
    col = torch.tensor([1.0, 2.0 ** -30, -1.0], device="cuda")
    x = torch.ones(3, 64, device="cuda")
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 2, 1], [1, 0, 2], [2, 1, 0]):
        go = col[order][:, None].contiguous()
        out, sv = G._forward(amd, net, x, False)
        assert bool((sv == 1.0).all()) and bool((out == 64.0).all())
        ex = Exact(amd, net, x, out, go, sv, False)
        assert torch.equal(ex.gsave[:3 * 64].view(3, 64), go.expand(3, 64))
        for got in (ex.w[0], ex.b[0], ex.w[1], ex.b[1]):
            assert bool((got == 2.0 ** -30).all()), (order, got.flatten()[:4])
        rw, rb, _ = _restate(net, 3, x, sv, ex.gsave, 30)
        for i in range(2):
            assert torch.equal(_bits(ex.w[i].cpu()), _bits(rw[i]["grad"])) and torch.equal(_bits(ex.b[i].cpu()), _bits(rb[i]["grad"]))
            assert bool((rw[i]["acc"] == 1 << 23).all()) and bool((rw[i]["emax"] == 127).all())


def test_poison(amd):
    """One Inf in grad_out (column 1 of row 40): the chain carries it into every dz of the hidden layers; in the output layer it
    reaches row 1 of the weights and element 1 of the bias alone."""
    cfg = CONFIGS[1]
    B = 65
    net = G.Net.get(cfg)
    x, go = G._inputs(net, B)
    out, sv = G._forward(amd, net, x, cfg[4])
    K = X.guard_bits(B)
    prev = _prefill(net, 3)
    clean = Exact(amd, net, x, out, go, sv, cfg[4], prev=([t.cuda() for t in prev[0]], [t.cuda() for t in prev[1]]))
    bad = go.clone()
    bad[40, 1] = float("inf")
    ex = Exact(amd, net, x, out, bad, sv, cfg[4], prev=([t.cuda() for t in prev[0]], [t.cuda() for t in prev[1]]))
    rw, rb, _ = _restate(net, B, x, sv, ex.gsave, K, prev=prev)
    for i in range(net.n_hidden + 1):
        for got, res in ((ex.w[i].cpu(), rw[i]), (ex.b[i].cpu(), rb[i])):
            nan = res["emax"] == 255
            assert torch.equal(torch.isnan(got), nan) and bool((_bits(got)[nan] == X.QNAN_BITS).all())
            assert torch.equal(_bits(got), _bits(res["grad"]))
    last = net.n_hidden
    nan_w, nan_b = torch.isnan(ex.w[last].cpu()), torch.isnan(ex.b[last].cpu())
    assert bool(nan_w[1].all()) and int(nan_w.sum()) == net.width and nan_b.tolist() == [False, True, False]
    assert bool(torch.isnan(ex.w[0]).any())
    keep = torch.tensor([0, 2])
    assert torch.equal(_bits(ex.w[last].cpu()[keep]), _bits(clean.w[last].cpu()[keep]))                      # as without the Inf
    assert torch.equal(_bits(ex.b[last].cpu()[keep]), _bits(clean.b[last].cpu()[keep]))


@pytest.mark.parametrize("cfg,B", CASES, ids=_CASE_IDS)
def test_accuracy_within_the_derived_bound(amd, cfg, B):
    c = _case(amd, cfg, B)
    net = c["net"]
    for i, (dz, inp) in enumerate(c["ops"]):
        tw, _, tb, _ = R.weight_grad(dz, inp)
        for kind, got, truth, res, operand in (("weights", c["ex"].w[i].cpu(), tw, c["rw"][i], inp), ("bias", c["ex"].b[i].cpu(), tb, c["rb"][i], None)):
            bound = X.error_bound(dz, operand, res["emax"], c["K"], truth)
            err = (got.double() - truth).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            _worst[f"{kind}_worst_error_over_bound"] = max(_worst.get(f"{kind}_worst_error_over_bound", 0.0), ratio)
            _worst["accumulator_peak_log2"] = max(_worst.get("accumulator_peak_log2", 0.0),
                                                  float(torch.log2(torch.tensor(float(max(1, res["max_abs_acc"]))))))
            assert bool((err <= bound).all()), f"{kind} of layer {i} at B={B}: error above the bound (worst ratio {ratio:.3f})"
            assert res["max_abs_acc"] < 2 ** 63
    print(f"    {_IDS[CONFIGS.index(cfg)]} B={B}: worst so far {dict((k, round(v, 3)) for k, v in _worst.items())}")


def test_refusals_write_nothing(amd):
    L = amd._lib
    lib = L.load()
    cfg = CONFIGS[1]
    c = _case(amd, cfg, 33)
    net, B = c["net"], 33
    gr = G.Grads(net, B)
    ws_whole, ws, need = _workspace(amd, net)
    st = L.stream_of(c["x"].device)
    gw, gb = G._ptrs([t[1] for t in gr.w]), G._ptrs([t[1] for t in gr.b])

    def call(ws_p=ws.data_ptr(), nbytes=need, B=B, width=net.width, gw=gw):
        rc = lib.nerf_fused_mlp_backward_exact(c["x"].data_ptr(), c["out"].data_ptr(), c["go"].data_ptr(), B, net.in_dim, width, net.n_hidden,
                                               net.out_dim, 0, G._ptrs(net.w), c["sv"].data_ptr(), gr.gsave.data_ptr(), gw, gb,
                                               gr.gx.data_ptr(), ws_p, nbytes, st)
        assert rc != 0 and "nerf_fused_mlp_backward_exact" in lib.nerf_last_error().decode()
        return rc
    assert call(ws_p=None) == -1 and call(ws_p=ws.data_ptr() + 8) == -1 and call(B=0) == -1 and call(gw=None) == -1
    assert call(nbytes=need - 1) == -2 and call(nbytes=0) == -2 and call(width=96) == -4
    torch.cuda.synchronize()
    assert bool((gr.gsave == G.SENTINEL).all()) and bool((gr.gx == G.SENTINEL).all())       # not even the chain ran
    assert all(bool((t[1] == 0).all()) for t in gr.w + gr.b)
    assert bool((ws_whole == WS_SENTINEL).all())                           # nor the zero-fill


# ---- the module ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [CONFIGS[1], CONFIGS[2]], ids=[_IDS[1], _IDS[2]])
def test_autograd_equals_the_direct_call(amd, cfg):
    B = ROWS_PER_WORKGROUP + 1
    c = _case(amd, cfg, B)
    net, direct = c["net"], c["ex"]
    act = "sigmoid" if cfg[4] else None
    n = net.n_hidden + 1
    # fused_mlp: every gradient, then the parameters alone
    w, b = [t.clone().requires_grad_(True) for t in net.w], [t.clone().requires_grad_(True) for t in net.b]
    xr = c["x"].clone().requires_grad_(True)
    out = amd.fused_mlp(xr, w, b, act, deterministic=True)
    assert torch.equal(out.detach(), c["out"])
    grads = torch.autograd.grad(out, w + b + [xr], c["go"])
    for i in range(n):
        assert torch.equal(_bits(grads[i]), _bits(direct.w[i])) and torch.equal(_bits(grads[n + i]), _bits(direct.b[i])), i
    assert torch.equal(grads[-1], direct.gx.view(B, net.in_dim))
    grads = torch.autograd.grad(amd.fused_mlp(c["x"], w, b, act, deterministic=True), w + b, c["go"])
    assert all(torch.equal(_bits(grads[i]), _bits(direct.w[i])) and torch.equal(_bits(grads[n + i]), _bits(direct.b[i])) for i in range(n))
    # one bias alone; a frozen network: the input gradient alone
    (g1,) = torch.autograd.grad(amd.fused_mlp(c["x"], net.w, [net.b[0], b[1]] + net.b[2:], act, deterministic=True), (b[1],), c["go"])
    assert torch.equal(_bits(g1), _bits(direct.b[1]))
    (gx,) = torch.autograd.grad(amd.fused_mlp(xr, net.w, net.b, act, deterministic=True), (xr,), c["go"])
    assert torch.equal(gx, direct.gx.view(B, net.in_dim))
    # FusedMLP, prefix shape [5, 205, in_dim]
    mod = amd.FusedMLP(net.in_dim, net.out_dim, net.width, net.n_hidden, act, deterministic=True).cuda()
    with torch.no_grad():
        for layer, wi, bi in zip(mod.layers, net.w, net.b):
            layer.weight.copy_(wi)
            layer.bias.copy_(bi)
    mod(c["x"].view(5, 205, net.in_dim)).backward(c["go"].view(5, 205, net.out_dim))
    for i, layer in enumerate(mod.layers):
        assert torch.equal(_bits(layer.weight.grad), _bits(direct.w[i])) and torch.equal(_bits(layer.bias.grad), _bits(direct.b[i]))


def test_image_fit_network_hands_the_flag_on(amd):
    from nerf_replication_amd.fused_mlp import frequency_encode
    torch.manual_seed(1)
    model = amd.ImageFitNetwork(D=2, W=64, deterministic=True).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    uv = torch.rand(1500, 2, device="cuda", generator=gen)
    go = torch.randn(1500, 3, device="cuda", generator=gen)
    model.render(uv)["rgb"].backward(go)
    layers = list(model.backbone_layer) + [model.output_layer[0]]
    net = G.Net.__new__(G.Net)
    net.in_dim, net.width, net.n_hidden, net.out_dim, net.sigmoid = 42, 64, 2, 3, True
    net.w, net.b = [l.weight.detach() for l in layers], [l.bias.detach() for l in layers]
    x = frequency_encode(uv, 10).contiguous()
    out, sv = G._forward(amd, net, x, True)
    direct = Exact(amd, net, x, out, go, sv, True)
    for i, layer in enumerate(layers):
        assert torch.equal(_bits(layer.weight.grad), _bits(direct.w[i])) and torch.equal(_bits(layer.bias.grad), _bits(direct.b[i]))
        assert float(direct.w[i].abs().max()) > 0


def _small_field(amd, seed=0, deterministic=True):
    torch.manual_seed(seed)
    enc = amd.HashEncoder(input_dim=3, num_levels=4, level_dim=2, per_level_scale=2, base_resolution=8, log2_hashmap_size=12,
                          deterministic=deterministic)
    field = amd.HashField((-2.0, -2.0, -2.0, 2.0, 2.0, 2.0), encoder=enc, deterministic=deterministic).cuda()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5, generator=None)       # (the default init is 1e-4: a flat field)
    return field


def test_hashfield_density_hands_the_flag_on(amd, monkeypatch):
    from nerf_replication_amd import hashfield
    seen = []
    real = hashfield.fused_mlp

    def spy(x, weights, biases, output_activation=None, deterministic=False):
        out = real(x, weights, biases, output_activation, deterministic)
        seen.append([deterministic, x.detach().clone(), None])
        out.register_hook(lambda g, rec=seen[-1]: rec.__setitem__(2, g.detach().clone()))
        return out
    monkeypatch.setattr(hashfield, "fused_mlp", spy)
    field = _small_field(amd)
    xyz = (torch.rand(1100, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) - 0.5) * 3.8
    field.density(xyz).sum().backward()
    assert [s[0] for s in seen] == [True]
    layers = field.sigma_net.layers
    net = G.Net.__new__(G.Net)
    net.in_dim, net.width, net.n_hidden, net.out_dim, net.sigmoid = 8, 64, 1, 16, False
    net.w, net.b = [l.weight.detach() for l in layers], [l.bias.detach() for l in layers]
    x, go = seen[0][1].contiguous(), seen[0][2].contiguous()
    out, sv = G._forward(amd, net, x, False)
    direct = Exact(amd, net, x, out, go, sv, False)
    for i, layer in enumerate(layers):
        assert torch.equal(_bits(layer.weight.grad), _bits(direct.w[i])) and torch.equal(_bits(layer.bias.grad), _bits(direct.b[i]))
    assert float(direct.w[0].abs().max()) > 0


def _rays(n, seed):
    """n rays from a sphere of radius 4 towards points near the origin, and a smooth colour per ray."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=1) * 4.0
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen) * 0.5 - o, dim=1)
    colors = 0.5 + 0.5 * torch.sin(3.0 * d + torch.tensor([0.0, 1.0, 2.0]))
    return o.cuda().contiguous(), d.cuda().contiguous(), colors.cuda().contiguous()


def _train(amd, rays, steps, with_grid):
    from nerf_replication_amd.training import FusedAdam, train_step
    field = _small_field(amd, seed=3)
    ren = amd.HashRenderer(field)
    ren.N_samples = 32
    if with_grid:                                                          # a hand-made grid: the half of the box with x < 0 is occupied
        half = -torch.ones(17, 17, 17)
        half[:8] = 1.0
        ren.occupancy = amd.OccupancyGrid.from_fields(field.bbox, fine=half.cuda(), level=0.0, dilate=0)
        ren.stats = []
    opt = FusedAdam(field.parameters(), lr=1e-2)
    losses = torch.stack([train_step(ren, opt, *rays) for _ in range(steps)])
    return [p.detach().clone() for p in field.parameters()], losses, ren.stats


@pytest.mark.parametrize("with_grid", [False, True], ids=["plain", "occupancy"])
def test_training_a_hashfield_twice_gives_the_same_bytes(amd, with_grid):
    rays = _rays(256, seed=11)
    params_a, loss_a, stats = _train(amd, rays, 20, with_grid)
    params_b, loss_b, _ = _train(amd, rays, 20, with_grid)
    print(f"    loss {float(loss_a[0]):.5f} -> {float(loss_a[-1]):.5f}" + (f", evaluated {sum(m for m, _ in stats)} of "
                                                                          f"{sum(p for _, p in stats)} samples" if with_grid else ""))
    assert len(params_a) == 11 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(params_a, params_b))
    assert torch.equal(_bits(loss_a), _bits(loss_b))
    assert bool(torch.isfinite(loss_a).all()) and float(loss_a[-1]) < float(loss_a[0])
    if with_grid:
        kept = sum(m for m, _ in stats) / sum(p for _, p in stats)
        assert 0.2 < kept < 0.8 and len(stats) == 20                       # the grid culls a real share, in every step


def test_parameter_gradients_do_not_depend_on_the_order_of_the_rays(amd):
    """One chunk of 256 rays x 32 samples: a permutation of the rays permutes the rows of every network call, the MSE's gradient
    is per element, compositing per ray."""
    o, d, colors = _rays(256, seed=12)
    field = _small_field(amd, seed=5)
    ren = amd.HashRenderer(field)
    ren.N_samples = 32

    def grads(order):
        field.zero_grad(set_to_none=True)
        rgb, _ = ren.render({"rays_o": o[order][None].contiguous(), "rays_d": d[order][None].contiguous()})
        torch.nn.functional.mse_loss(rgb, colors[order]).backward()
        return {k: p.grad.clone() for k, p in field.named_parameters()}
    first = grads(torch.arange(256, device="cuda"))
    assert len(first) == 11 and all(float(g.abs().max()) > 0 for g in first.values())
    for seed in (1, 2):
        moved = grads(torch.randperm(256, generator=torch.Generator().manual_seed(seed)).cuda())
        for k in first:
            assert torch.equal(_bits(first[k]), _bits(moved[k])), (seed, k)
