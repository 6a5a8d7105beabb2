"""GPU tests of the fused MLP entries (csrc/nerf_fused_mlp.hip.inc, include/nerf_mi355x_nn.h) against the float64 restatement in
tests/fused_mlp_reference.py.

Bounds (u = 2^-24).  All of them are derived, none measured; they hold for any summation order, because an fp32 fma / MFMA / atomic sum
of n terms in any order errs by at most (n - 1) roundings of partial sums that never exceed sum|term| (plus the rounding of the
result).  Every check starts from the KERNEL'S OWN fp32 operands (its saved rows), so errors do not compound and no ReLU decision can
differ.  No element is exempt.
  forward, per layer     |got - relu(truth)| <= (K + 2) u (sum_k |w_k in_k| + |b|), K the layer's true input width; the same for z from
                         the saved last hidden row when the activation is none
  sigmoid                |y - sigmoid64(z)| <= 8 u with z from the same configuration run with activation none: exp to 3 ulp and the
                         division to 2.5 ulp (OpenCL's bounds), one add and the roundings; the function's condition number is at most 1
                         and y <= 1, so ulps are absolute.  z = +-100 gives exactly 1, or a finite value within 8 u of 0
  dz_out                 bit-equal to grad_out (none); within 4 u |truth| of g y (1 - y) (sigmoid: three roundings)
  dz_i, grad_x           |got - truth| <= (K_out + 1) u sum_o |w dz_{i+1}|; exactly 0 where the saved h_i is 0
  grad_W[o,k]            <= (n + 2) u sum_p |dz[p,o] in[p,k]|,  grad_b[o] <= (n + 1) u sum_p |dz[p,o]|, n = B, or 2 B after a second call
                         into the same buffers
Every buffer the entries write is the interior of a larger sentinel-filled one; the sentinels must be intact afterwards.  The worst
error / bound ratio per quantity goes to profiles/fused_mlp_parity.json."""
import ctypes

import pytest
import torch

import fused_mlp_reference as R
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

U = R.U
SENTINEL, PAD = -77.0, 8            # PAD floats = 32 bytes: the interior keeps the 16-byte alignment save and gsave need
BATCHES = (1, 31, 32, 33, 65, 4113)
#          in_dim width n_hidden out_dim sigmoid
CONFIGS = [(1, 64, 1, 1, False), (2, 64, 2, 3, True), (31, 64, 2, 16, False), (32, 128, 4, 3, True), (42, 128, 4, 3, True),
           (256, 128, 1, 4, False), (32, 64, 8, 3, False)]
_IDS = ["%dx%dx%d-%d%s" % (c[0], c[1], c[2], c[3], "-sigmoid" if c[4] else "") for c in CONFIGS]
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _keep_the_figures():
    """Keeps the worst error / bound ratio of every quantity the tests of this module measured (profiles/fused_mlp_parity.json)."""
    yield
    if _worst:
        R.parity_record("fused_mlp_bounds", {k: round(v, 4) for k, v in sorted(_worst.items())})


def _padded(n, zero=False):
    whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    inner = whole[PAD:PAD + n]
    if zero:
        inner.zero_()
    return whole, inner


def _intact(whole, n):
    return bool((whole[:PAD] == SENTINEL).all() and (whole[PAD + n:] == SENTINEL).all())


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class Net:
    """One configuration: seeded parameters on the GPU (made once per module)."""
    _cache = {}

    def __init__(self, cfg):
        self.in_dim, self.width, self.n_hidden, self.out_dim, self.sigmoid = cfg
        w, b = R.make_params(self.in_dim, self.width, self.n_hidden, self.out_dim, seed=sum(cfg[:4]))
        self.w, self.b = [t.cuda() for t in w], [t.cuda() for t in b]

    @classmethod
    def get(cls, cfg):
        if cfg not in cls._cache:
            cls._cache[cfg] = cls(cfg)
        return cls._cache[cfg]

    def dims(self, B):
        return (B, self.in_dim, self.width, self.n_hidden, self.out_dim)

    def layer_shape(self, i):
        return (self.out_dim if i == self.n_hidden else self.width, self.width if i else self.in_dim)


def _forward(amd, net, x, sigmoid, save=True):
    """-> (out [B, out_dim], save blocks [n_hidden, B, width] or None); the sentinels around both are checked."""
    L = amd._lib
    B = x.shape[0]
    whole_o, out = _padded(B * net.out_dim)
    n_save = net.n_hidden * B * net.width
    whole_s, sv = _padded(n_save) if save else (None, None)
    L.call("nerf_fused_mlp_forward", x, *net.dims(B), int(sigmoid), net.w, net.b, out, sv if save else None)
    assert _intact(whole_o, B * net.out_dim) and (not save or _intact(whole_s, n_save))
    assert not (out == SENTINEL).any() and (not save or not (sv == SENTINEL).any())          # everything was written
    return out.view(B, net.out_dim), (sv.view(net.n_hidden, B, net.width) if save else None)


class Grads:
    """The buffers of one nerf_fused_mlp_backward call, each inside sentinels."""

    def __init__(self, net, B, want_x=True, skip_layers=()):
        self.net, self.B = net, B
        self.n_gsave = net.n_hidden * B * net.width + B * net.out_dim
        self.whole_g, self.gsave = _padded(self.n_gsave)
        self.whole_x, self.gx = _padded(B * net.in_dim)
        self.want_x, self.skip = want_x, set(skip_layers)
        self.w, self.b = [], []
        for i in range(net.n_hidden + 1):
            n_out, n_in = net.layer_shape(i)
            self.w.append(_padded(n_out * n_in, zero=i not in self.skip))
            self.b.append(_padded(n_out, zero=i not in self.skip))

    def call(self, amd, x, out, go, sv, sigmoid):
        L, net = amd._lib, self.net
        gw = [None if i in self.skip else t[1] for i, t in enumerate(self.w)]
        gb = [None if i in self.skip else t[1] for i, t in enumerate(self.b)]
        L.call("nerf_fused_mlp_backward", x, out, go, *net.dims(self.B), int(sigmoid), net.w, sv, self.gsave, gw, gb,
               self.gx if self.want_x else None)
        assert _intact(self.whole_g, self.n_gsave) and _intact(self.whole_x, self.B * net.in_dim)
        for i in range(net.n_hidden + 1):
            n_out, n_in = net.layer_shape(i)
            assert _intact(self.w[i][0], n_out * n_in) and _intact(self.b[i][0], n_out)

    def dz(self, i):
        net, B = self.net, self.B
        if i == net.n_hidden:
            return self.gsave[net.n_hidden * B * net.width:].view(B, net.out_dim)
        return self.gsave[i * B * net.width:(i + 1) * B * net.width].view(B, net.width)


def _ratio(name, err, bound):
    """The worst error / bound of a quantity (0 / 0 counts as 0); kept per quantity for the parity file."""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(r.max()) if r.numel() else 0.0
    _worst[name] = max(_worst.get(name, 0.0), worst)
    return worst


def _inputs(net, B):
    x = R.make_inputs(B, net.in_dim, seed=B + net.in_dim).cuda()
    go = torch.randn(B, net.out_dim, generator=torch.Generator().manual_seed(B)).cuda()
    return x, go


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_forward_layer_by_layer(amd, cfg):
    net = Net.get(cfg)
    for B in BATCHES:
        x, _ = _inputs(net, B)
        z, sv = _forward(amd, net, x, sigmoid=False)
        inp = x
        for i in range(net.n_hidden):
            truth, mag = R.linear(inp, net.w[i], net.b[i])
            bound = (net.layer_shape(i)[1] + 2) * U * mag
            worst = _ratio("forward_hidden", (sv[i].double() - torch.relu(truth)).abs(), bound)
            print(f"{cfg} B={B} layer {i}: worst error/bound {worst:.3f}")
            assert worst <= 1.0, (B, i)
            inp = sv[i]
        truth, mag = R.linear(inp, net.w[-1], net.b[-1])
        worst = _ratio("forward_output", (z.double() - truth).abs(), (net.width + 2) * U * mag)
        print(f"{cfg} B={B} output: worst error/bound {worst:.3f}")
        assert worst <= 1.0, B
        # inference == SAVE forward, bit for bit
        assert torch.equal(_forward(amd, net, x, sigmoid=False, save=False)[0], z)
        if net.sigmoid:
            y, sv_y = _forward(amd, net, x, sigmoid=True)
            err = (y.double() - torch.sigmoid(z.double())).abs()
            print(f"{cfg} B={B} sigmoid: worst error {float(err.max()) / U:.3f} u")
            assert _ratio("sigmoid", err, torch.full_like(err, 8 * U)) <= 1.0
            assert torch.equal(sv_y, sv) and torch.equal(_forward(amd, net, x, sigmoid=True, save=False)[0], y)


def test_sigmoid_saturates_cleanly(amd):
    """z = +100 gives exactly 1, z = -100 a finite value within 8 u of 0, z = 0 exactly 0.5."""
    net = Net.get(CONFIGS[1])
    x, _ = _inputs(net, 33)
    flat = Net(CONFIGS[1])
    flat.w = net.w[:-1] + [torch.zeros_like(net.w[-1])]
    flat.b = net.b[:-1] + [torch.tensor([100.0, -100.0, 0.0], device="cuda")]
    y, _ = _forward(amd, flat, x, sigmoid=True)
    assert torch.isfinite(y).all()
    assert (y[:, 0] == 1.0).all() and (y[:, 1].abs() <= 8 * U).all() and (y[:, 2] == 0.5).all()


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_position_invariance_and_reproducibility(amd, cfg):
    """A row's result does not depend on where it sits in the batch (tails, tiles, workgroups), nor on the alignment of x."""
    net = Net.get(cfg)
    x, go = _inputs(net, 4113)
    rows = [0, 31, 32, 4095, 4096, 4112]
    out, sv = _forward(amd, net, x, net.sigmoid)
    out_rows, sv_rows = _forward(amd, net, x[rows].contiguous(), net.sigmoid)
    assert torch.equal(out_rows, out[rows]) and torch.equal(sv_rows, sv[:, rows])
    # x one float off its 16-byte alignment: the one-float-at-a-time input path, the same values
    shifted = torch.empty(x.numel() + 1, device="cuda")[1:].view_as(x).copy_(x)
    assert shifted.data_ptr() % 16 == 4
    out_s, sv_s = _forward(amd, net, shifted, net.sigmoid)
    assert torch.equal(out_s, out) and torch.equal(sv_s, sv)
    # two runs: bit-identical out, save, gsave and grad_x
    g1, g2 = Grads(net, 4113), Grads(net, 4113)
    g1.call(amd, x, out, go, sv, net.sigmoid)
    out2, sv2 = _forward(amd, net, x, net.sigmoid)
    g2.call(amd, x, out2, go, sv2, net.sigmoid)
    assert torch.equal(out2, out) and torch.equal(sv2, sv)
    assert torch.equal(g1.gsave, g2.gsave) and torch.equal(g1.gx, g2.gx)
    # the gradient chain of a row does not depend on its position either
    g3 = Grads(net, len(rows))
    g3.call(amd, x[rows].contiguous(), out_rows, go[rows].contiguous(), sv_rows.contiguous(), net.sigmoid)
    assert torch.equal(g3.gx.view(len(rows), -1), g1.gx.view(4113, -1)[rows])
    for i in range(net.n_hidden + 1):
        assert torch.equal(g3.dz(i), g1.dz(i)[rows])


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_backward_layer_by_layer(amd, cfg):
    net = Net.get(cfg)
    for B in BATCHES:
        x, go = _inputs(net, B)
        out, sv = _forward(amd, net, x, net.sigmoid)
        g = Grads(net, B)
        g.call(amd, x, out, go, sv, net.sigmoid)
        assert not (g.gsave == SENTINEL).any() and not (g.gx == SENTINEL).any()
        # dz_out
        truth = R.dz_out(go, out, net.sigmoid)
        if net.sigmoid:
            assert _ratio("dz_out", (g.dz(net.n_hidden).double() - truth).abs(), 4 * U * truth.abs()) <= 1.0
        else:
            assert torch.equal(g.dz(net.n_hidden), go)
        # the chain, from the kernel's own dz of the layer above
        for i in range(net.n_hidden - 1, -1, -1):
            truth, mag = R.transposed(g.dz(i + 1), net.w[i + 1])
            live = sv[i] > 0
            k_out = net.layer_shape(i + 1)[0]
            worst = _ratio("dz_hidden", (g.dz(i).double() - truth * live).abs(), (k_out + 1) * U * mag * live)
            print(f"{cfg} B={B} dz_{i}: worst error/bound {worst:.3f}")
            assert worst <= 1.0, (B, i)
            assert (g.dz(i)[~live] == 0).all()
        truth, mag = R.transposed(g.dz(0), net.w[0])
        worst = _ratio("grad_x", (g.gx.view(B, -1).double() - truth).abs(), (net.width + 1) * U * mag)
        print(f"{cfg} B={B} grad_x: worst error/bound {worst:.3f}")
        assert worst <= 1.0, B
        # weight and bias gradients, after one call and after a second one into the same buffers
        for n_calls in (1, 2):
            if n_calls == 2:
                g.call(amd, x, out, go, sv, net.sigmoid)
            n = n_calls * B
            for i in range(net.n_hidden + 1):
                n_out, n_in = net.layer_shape(i)
                dw, dw_mag, db, db_mag = R.weight_grad(g.dz(i), x if i == 0 else sv[i - 1])
                w_worst = _ratio("grad_weight", (g.w[i][1].view(n_out, n_in).double() - n_calls * dw).abs(), (n + 2) * U * n_calls * dw_mag)
                b_worst = _ratio("grad_bias", (g.b[i][1].double() - n_calls * db).abs(), (n + 1) * U * n_calls * db_mag)
                print(f"{cfg} B={B} call {n_calls} layer {i}: grad_W {w_worst:.3f} grad_b {b_worst:.3f} of the bound")
                assert w_worst <= 1.0 and b_worst <= 1.0, (B, i, n_calls)


@pytest.mark.parametrize("cfg", [CONFIGS[3], CONFIGS[2]], ids=[_IDS[3], _IDS[2]])
def test_optional_gradients_are_left_alone(amd, cfg):
    """grad_x = NULL: its buffer stays all sentinel.  A layer whose gradient pointers are both NULL: its buffers stay untouched, and
    the other layers get what they get in a full call."""
    net = Net.get(cfg)
    B = 65
    x, go = _inputs(net, B)
    out, sv = _forward(amd, net, x, net.sigmoid)
    full = Grads(net, B)
    full.call(amd, x, out, go, sv, net.sigmoid)
    skip = (1, net.n_hidden)
    part = Grads(net, B, want_x=False, skip_layers=skip)
    part.call(amd, x, out, go, sv, net.sigmoid)
    assert (part.whole_x == SENTINEL).all()
    assert torch.equal(part.gsave, full.gsave)
    for i in range(net.n_hidden + 1):
        n_out, n_in = net.layer_shape(i)
        if i in skip:
            assert (part.w[i][0] == SENTINEL).all() and (part.b[i][0] == SENTINEL).all()
        else:       # atomics: equal up to the order-free bound, twice (both sides carry it)
            dw, dw_mag, db, db_mag = R.weight_grad(full.dz(i), x if i == 0 else sv[i - 1])
            assert ((part.w[i][1].view(n_out, n_in).double() - dw).abs() <= (B + 2) * U * dw_mag).all()
            assert ((part.b[i][1].double() - db).abs() <= (B + 1) * U * db_mag).all()


def test_refusals_at_the_c_level(amd):
    """Refused before any launch: the documented status, a message, and nothing written."""
    L = amd._lib
    net = Net.get(CONFIGS[1])
    x, _ = _inputs(net, 33)
    B, in_dim, width, n_hidden, out_dim = net.dims(33)
    cases = [((B, in_dim, 96, n_hidden, out_dim), x, -4), ((B, in_dim, width, n_hidden, 17), x, -4),
             ((0, in_dim, width, n_hidden, out_dim), x, -1), ((B, in_dim, width, n_hidden, out_dim), None, -1)]
    for dims, xin, status in cases:
        whole_o, out = _padded(B * 17)
        whole_s, sv = _padded(n_hidden * B * 128)
        rc = L.load().nerf_fused_mlp_forward(None if xin is None else xin.data_ptr(), *dims, 1, _ptrs(net.w), _ptrs(net.b),
                                             out.data_ptr(), sv.data_ptr(), L.stream_of(x.device))
        torch.cuda.synchronize()
        assert rc == status, (dims, rc)
        assert L.load().nerf_last_error().decode().startswith("nerf_fused_mlp_forward: ")
        assert (whole_o == SENTINEL).all() and (whole_s == SENTINEL).all()
        whole_g, gsave = _padded(n_hidden * B * 128 + B * 17)
        whole_x, gx = _padded(B * in_dim)
        gw = [_padded(128 * 128)[1] for _ in range(n_hidden + 1)]
        rc = L.load().nerf_fused_mlp_backward(None if xin is None else xin.data_ptr(), out.data_ptr(), out.data_ptr(), *dims, 1,
                                              _ptrs(net.w), sv.data_ptr(), gsave.data_ptr(), _ptrs(gw), _ptrs([None] * (n_hidden + 1)),
                                              gx.data_ptr(), L.stream_of(x.device))
        torch.cuda.synchronize()
        assert rc == status, (dims, rc)
        assert L.load().nerf_last_error().decode().startswith("nerf_fused_mlp_backward: ")
        assert (whole_g == SENTINEL).all() and (whole_x == SENTINEL).all() and all((t == SENTINEL).all() for t in gw)
    rc = L.load().nerf_fused_mlp_forward(x.data_ptr(), B, in_dim, 96, n_hidden, out_dim, 0, _ptrs(net.w), _ptrs(net.b), None, None, None)
    with pytest.raises(L.NerfLibraryError, match="width must be 64 or 128"):
        L.check(rc, "nerf_fused_mlp_forward")
