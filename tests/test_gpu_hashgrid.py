"""GPU tests of the hash-grid encoding (csrc/nerf_hashgrid.hip.inc, nerf_replication_amd/hashgrid.py) against the restatement in
tests/hashgrid_reference.py.

What is asserted, and where the bounds come from:
  forward        bit-equal to the fp32 fixed-order restatement: the same operations in the same order, contraction off.
  grad_emb       per element |got - truth| <= (k + 2D + 2) * 2^-24 * sum|term|, k = number of contributions to the element, sum|term|
                 their absolute sum in float64: an fp32 sum of k terms in ANY order errs by at most (k - 1) roundings of partial sums
                 that never exceed sum|term|, and a term w * grad_out carries at most D roundings of 1 - f, D - 1 multiplies and the
                 final product (2D <= 2D + 2).  It holds whatever order the atomics arrive in.  Untouched entries stay exactly 0.
  accumulation   a second call into the same buffer: 2k terms with the absolute sum 2 * sum|term|, the same form of bound.
  grad_x         the same form over its own terms grad_out * scale * prod(other factors) * (emb[right] - emb[left]): at most D - 1
                 roundings of 1 - f, D - 1 multiplies, the difference, and two products (2D + 1 <= 2D + 2).
Every buffer the kernels write is the interior of a larger sentinel-filled one; the sentinels must be intact afterwards."""
import ctypes

import numpy as np
import pytest
import torch

import hashgrid_reference as R
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL, PAD = -77.0, 8            # PAD floats = 32 bytes: the interior keeps the 4*C-byte alignment the entries ask for
BATCHES = (1, 63, 64, 65, 513, 4096)
#            D  L   C  s    H   T
CONFIGS = {
    "default": (3, 16, 2, 2, 16, 19),          # including the wrapped-dense levels 12 and 13
    "dense0_2d": (2, 4, 2, 2, 15, 19),         # dense level 0
    "dense_then_hashed": (3, 4, 2, 2, 15, 12),  # dense, then three hashed levels of one size
    "d4_contended": (4, 2, 2, 2, 3, 8),        # 16 corners, 256-row tables: the heaviest contention
    "c1": (2, 3, 1, 1.5, 7, 8),                # C = 1, two dense levels
    "c4": (3, 3, 4, 1.5, 3, 6),                # C = 4
    "c8": (3, 2, 8, 2, 5, 9),                  # C = 8: a dense level of 6^3 = 216 rows and a hashed one of 512
}


class Case:
    """One configuration: its level table and a random table on the GPU (made once per module)."""
    _cache = {}

    def __init__(self, name):
        self.D, self.L, self.C, self.s, self.H, self.T = CONFIGS[name]
        self.off = R.level_offsets(self.D, self.L, self.s, self.H, self.T)
        self.sc = R.level_scales(self.L, self.s, self.H)
        gen = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
        self.emb = torch.rand(self.off[-1], self.C, generator=gen, device="cuda") * 2 - 1
        self.off_c = (ctypes.c_int32 * (self.L + 1))(*self.off)
        self.sc_c = (ctypes.c_float * self.L)(*[float(v) for v in self.sc])

    @classmethod
    def get(cls, name):
        if name not in cls._cache:
            cls._cache[name] = cls(name)
        return cls._cache[name]

    def inputs(self, B, seed=0):
        x = R.make_inputs(B, self.D, self.H, seed=seed + B).cuda()
        gen = torch.Generator(device="cuda").manual_seed(B)
        go = torch.randn(B, self.L * self.C, generator=gen, device="cuda")
        return x, go


def _padded(n, zero=False):
    whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    inner = whole[PAD:PAD + n]
    if zero:
        inner.zero_()
    return whole, inner


def _intact(whole, n):
    return bool((whole[:PAD] == SENTINEL).all() and (whole[PAD + n:] == SENTINEL).all())


def _forward(amd, cs, x, emb=None):
    L = amd._lib
    emb = cs.emb if emb is None else emb
    B = x.shape[0]
    whole, out = _padded(B * cs.L * cs.C)
    L.call("nerf_hashgrid_forward", x, emb, B, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c, out)
    torch.cuda.synchronize()
    assert _intact(whole, B * cs.L * cs.C)
    return out.view(B, cs.L * cs.C)


def _backward(amd, cs, x, go, want_emb=True, want_x=True, into=None):
    """-> (grad_emb, grad_x, buffers); `into`: the buffers of an earlier call, to accumulate into the same grad_emb."""
    L = amd._lib
    B = x.shape[0]
    ne, nx = cs.emb.numel(), B * cs.D
    we, ge = into[0] if into else _padded(ne, zero=True)
    wx, gx = _padded(nx)
    L.call("nerf_hashgrid_backward", x, cs.emb, go, B, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c, ge if want_emb else None, gx if want_x else None)
    torch.cuda.synchronize()
    assert _intact(we, ne) and _intact(wx, nx)
    if not want_x:
        assert bool((gx == SENTINEL).all())
    if not want_emb and not into:
        assert bool((ge == 0).all())
    return ge.view_as(cs.emb), gx.view(B, cs.D), ((we, ge),)


def _within(got, truth, abs_sum, count, D, what, terms=1):
    """|got - terms * truth| <= (terms * count + 2D + 2) * 2^-24 * terms * abs_sum, element by element; prints the worst ratio."""
    err = (got.double() - terms * truth).abs()
    bound = (terms * count + 2 * D + 2) * U * terms * abs_sum
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"    {what}: max err / bound = {ratio:.3f}, max err {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: error above the bound (worst ratio {ratio:.3f})"


# ---- forward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_bit_equal(amd, name):
    cs = Case.get(name)
    for B in BATCHES:
        x, _ = cs.inputs(B)
        got = _forward(amd, cs, x)
        ref = R.forward_f32(x, cs.emb, cs.off, cs.sc)
        same = got.view(torch.int32) == ref.view(torch.int32)
        print(f"    {name} B={B}: {int((~same).sum())} of {same.numel()} differ")
        assert bool(same.all())
        assert bool(ref.abs().max() > 0.01)                               # (the comparison is not of zeros)


# ---- gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_gradients_within_the_fp32_bound(amd, name):
    cs = Case.get(name)
    for B in BATCHES:
        x, go = cs.inputs(B)
        t = R.truth_f64(x, cs.emb, cs.off, cs.sc, go)
        ge, gx, bufs = _backward(amd, cs, x, go)
        print(f"  {name} B={B}")
        _within(ge, t["grad_emb"], t["grad_emb_abs"], t["grad_emb_count"], cs.D, "grad_emb")
        assert bool((ge[t["grad_emb_count"] == 0] == 0).all())            # entries that nothing touches stay exactly 0
        assert float(ge.abs().max()) > 0
        _within(gx, t["grad_x"], t["grad_x_abs"], t["grad_x_count"], cs.D, "grad_x")
        # the entry accumulates: a second call into the same buffer gives twice the gradient
        ge2, _, _ = _backward(amd, cs, x, go, want_x=False, into=bufs)
        _within(ge2, t["grad_emb"], t["grad_emb_abs"], t["grad_emb_count"], cs.D, "grad_emb, two calls", terms=2)
        assert bool((ge2[t["grad_emb_count"] == 0] == 0).all())


@pytest.mark.parametrize("name", ["dense_then_hashed", "d4_contended"])
def test_identical_points_add_into_the_same_rows(amd, name):
    cs = Case.get(name)
    B = 4096
    x = torch.rand(1, cs.D, generator=torch.Generator().manual_seed(5)).expand(B, cs.D).contiguous().cuda()
    go = torch.randn(B, cs.L * cs.C, generator=torch.Generator(device="cuda").manual_seed(6), device="cuda")
    # (the truth on the CPU: float64 index_add_ with 4096 equal indices is slow on the GPU)
    t = {k: v.cuda() for k, v in R.truth_f64(x.cpu(), cs.emb.cpu(), cs.off, cs.sc, go.cpu()).items()}
    touched = t["grad_emb_count"] > 0
    assert float(t["grad_emb_count"].max()) >= B and int(touched[:, 0].sum()) <= cs.L * 2 ** cs.D
    ge, gx, _ = _backward(amd, cs, x, go)
    _within(ge, t["grad_emb"], t["grad_emb_abs"], t["grad_emb_count"], cs.D, "grad_emb")
    assert bool((ge[~touched] == 0).all())
    _within(gx, t["grad_x"], t["grad_x_abs"], t["grad_x_count"], cs.D, "grad_x")
    got = _forward(amd, cs, x)
    assert bool((got == got[0]).all()) and torch.equal(got, R.forward_f32(x, cs.emb, cs.off, cs.sc))


def test_only_what_is_asked_for_is_written(amd):
    cs = Case.get("dense_then_hashed")
    x, go = cs.inputs(65)
    ge, _, _ = _backward(amd, cs, x, go, want_x=False)                    # (the helper checks that grad_x stayed sentinel)
    _, gx, _ = _backward(amd, cs, x, go, want_emb=False)                  # (... and that grad_emb stayed zero)
    ge_b, gx_b, _ = _backward(amd, cs, x, go)
    assert torch.equal(gx, gx_b)                                          # no atomics in the input gradient: the same bytes
    t = R.truth_f64(x, cs.emb, cs.off, cs.sc, go)
    _within(ge, t["grad_emb"], t["grad_emb_abs"], t["grad_emb_count"], cs.D, "grad_emb alone")


def test_inputs_outside_the_domain_stay_inside_the_level(amd):
    """normalize=False with out-of-range and non-finite inputs: unspecified values, but every row is reduced modulo n -- the rows of
    the batch that are in range come out as ever, and nothing outside the buffers is written."""
    for name in ("default", "d4_contended"):
        cs = Case.get(name)
        x, go = cs.inputs(64)
        bad = torch.tensor([-1.0, 2.0, float("inf"), float("-inf"), float("nan"), 1e30, -1e30, 3e9], device="cuda")
        x2 = x.clone()
        x2[8:16, :] = bad[:, None]
        x2[16:24, 0] = bad
        got = _forward(amd, cs, x2)
        ref = R.forward_f32(x, cs.emb, cs.off, cs.sc)
        keep = torch.ones(64, dtype=torch.bool, device="cuda")
        keep[8:24] = False
        assert torch.equal(got[keep], ref[keep])
        ge, gx, _ = _backward(amd, cs, x2, go)                            # (sentinels checked by the helper)
        assert bool(torch.isfinite(gx[keep]).all())


# ---- the module --------------------------------------------------------------------------------------------------------------------
def _encoder(amd, cs):
    enc = amd.HashEncoder(input_dim=cs.D, num_levels=cs.L, level_dim=cs.C, per_level_scale=cs.s, base_resolution=cs.H,
                          log2_hashmap_size=cs.T).cuda()
    assert enc.offsets.tolist() == cs.off
    with torch.no_grad():
        enc.embeddings.copy_(cs.emb)
    return enc


@pytest.mark.parametrize("name", ["dense_then_hashed", "c8"])
def test_autograd_equals_the_direct_calls(amd, name):
    cs = Case.get(name)
    enc = _encoder(amd, cs)
    x, go = cs.inputs(10)
    t = R.truth_f64(x, cs.emb, cs.off, cs.sc, go)
    _, gx_direct, _ = _backward(amd, cs, x, go)
    # prefix shape [2, 5, D], both gradients
    xr = x.view(2, 5, cs.D).clone().requires_grad_(True)
    out = enc(xr, normalize=False)
    assert out.shape == (2, 5, cs.L * cs.C) and torch.equal(out.detach().view(10, -1), _forward(amd, cs, x))
    gx, ge = torch.autograd.grad(out, (xr, enc.embeddings), go.view(2, 5, -1))
    assert torch.equal(gx.view(10, cs.D), gx_direct)
    _within(ge, t["grad_emb"], t["grad_emb_abs"], t["grad_emb_count"], cs.D, "autograd grad_emb")
    # an input that does not require grad gets no gradient, and the input-gradient kernel is not asked for
    out = enc(x, normalize=False)
    assert out.requires_grad
    (ge,) = torch.autograd.grad(out, (enc.embeddings,), go)
    _within(ge, t["grad_emb"], t["grad_emb_abs"], t["grad_emb_count"], cs.D, "autograd grad_emb, plain input")
    xn = x.clone().requires_grad_(True)
    out = enc(xn.detach(), normalize=False)
    assert torch.autograd.grad(out, (xn, enc.embeddings), go, allow_unused=True)[0] is None
    # a frozen table with an input that requires grad: the input gradient alone
    enc.embeddings.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    out = enc(xr, normalize=False)
    out.backward(go)
    assert torch.equal(xr.grad, gx_direct) and enc.embeddings.grad is None
    # neither requires grad: no graph
    assert not enc(x, normalize=False).requires_grad
    enc.embeddings.requires_grad_(True)
    # a non-contiguous input (a transposed view, and a column slice of a wider tensor)
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() or cs.D == 1
    wide = torch.cat([x, x], dim=1)[:, :cs.D]
    assert not wide.is_contiguous()
    for xin in (xt, wide):
        xin = xin.detach().requires_grad_(True)
        out = enc(xin, normalize=False)
        assert torch.equal(out.detach(), _forward(amd, cs, x))
        assert torch.equal(torch.autograd.grad(out, xin, go)[0], gx_direct)
    # double backward is refused, not answered with zeros
    xr = x.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(enc(xr, normalize=False), xr, go, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), xr)


def test_wbounds_normalisation(amd):
    cs = Case.get("dense_then_hashed")
    enc = _encoder(amd, cs)
    wb = torch.tensor([-1.0, -2.0, -0.5, 3.0, 1.0, 2.5], device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(9)
    xyz = (torch.rand(2, 5, 3, generator=gen, device="cuda") * 6 - 2.5)     # some points outside the box: clamped
    xyz[0, 0] = wb[:3]
    xyz[0, 1] = wb[3:]
    ext = float((wb[3:] - wb[:3]).max()) + 1e-6
    xr = xyz.clone().requires_grad_(True)
    norm = (torch.clamp(xr, min=wb[:3], max=wb[3:]) - wb[:3]) / ext
    assert float(norm.detach().min()) >= 0 and float(norm.detach().max()) <= 1
    out = enc(xyz, wb)                                                      # normalize=True is the default
    assert torch.equal(out.view(10, -1), _forward(amd, cs, norm.detach().view(10, 3).contiguous()))
    assert torch.equal(out, enc(xyz, wbounds=wb, normalize=True))
    # the gradient flows through the normalisation: d/dxyz = grad_x / ext inside the box, 0 where clamped
    go = torch.randn(2, 5, cs.L * cs.C, generator=gen, device="cuda")
    xq = xyz.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(enc(xq, wb), xq, go)
    _, gx_direct, _ = _backward(amd, cs, norm.detach().view(10, 3).contiguous(), go.view(10, -1).contiguous(), want_emb=False)
    (g_ref,) = torch.autograd.grad(norm, xr, gx_direct.view(2, 5, 3))
    assert torch.equal(g, g_ref)
    outside = (xyz < wb[:3]) | (xyz > wb[3:])
    assert bool(outside.any()) and bool((g[outside] == 0).all())


def test_triplane_is_three_2d_encoders(amd):
    tri = amd.TriPlane(num_levels=4, level_dim=2, base_resolution=15, log2_hashmap_size=10).cuda()
    wb = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], device="cuda")
    with torch.no_grad():
        for p in tri.parameters():
            p.uniform_(-1, 1)
    xyz = torch.rand(2, 33, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    out = tri(xyz, wb)
    assert out.shape == (2, 33, tri.out_dim) and tri.out_dim == 24
    norm = (torch.clamp(xyz, min=wb[:3], max=wb[3:]) - wb[:3]) / (1.0 + 1e-6)
    off, sc = R.level_offsets(2, 4, 2, 15, 10), R.level_scales(4, 2, 15)
    parts = [R.forward_f32(norm[..., ax].reshape(-1, 2), plane.embeddings.detach(), off, sc)
             for plane, ax in ((tri.xy_plane, [0, 1]), (tri.yz_plane, [1, 2]), (tri.xz_plane, [0, 2]))]
    assert torch.equal(out.reshape(-1, 24), torch.cat(parts, dim=1))
    planes = [tri.xy_plane(norm[..., [0, 1]], normalize=False), tri.yz_plane(norm[..., [1, 2]], normalize=False),
              tri.xz_plane(norm[..., [0, 2]], normalize=False)]
    assert torch.equal(out, torch.cat(planes, dim=-1))
    out.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in tri.parameters())


# ---- error paths -------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_are_refused_before_any_launch(amd):
    L = amd._lib
    lib = L.load()
    cs = Case.get("dense_then_hashed")
    x, go = cs.inputs(4)
    xw = torch.rand(4, 8, device="cuda")                                   # wide enough for any D tried
    off33 = (ctypes.c_int32 * 34)(*range(0, 34 * 8, 8))
    sc33 = (ctypes.c_float * 33)(*([1.0] * 33))
    whole, out = _padded(4 * 33 * 8)
    out.fill_(SENTINEL)
    we, ge = _padded(cs.emb.numel(), zero=True)
    st = L.stream_of(x.device)
    B31 = (1 << 31) // (cs.L * cs.C)                                       # B * L * C = 2^31: one past the 32-bit index range
    cases = {"D = 5": (4, 5, cs.C, cs.L, cs.off_c, cs.sc_c), "C = 3": (4, cs.D, 3, cs.L, cs.off_c, cs.sc_c),
             "L = 33": (4, cs.D, cs.C, 33, off33, sc33), "L = 0": (4, cs.D, cs.C, 0, cs.off_c, cs.sc_c),
             "B = 0": (0, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c), "B = -1": (-1, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c),
             "B*L*C = 2^31": (B31, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c)}
    for what, (B, D, C, Lv, off, sc) in cases.items():
        rc = lib.nerf_hashgrid_forward(xw.data_ptr(), cs.emb.data_ptr(), B, D, C, Lv, off, sc, out.data_ptr(), st)
        msg = lib.nerf_last_error().decode()
        assert rc != 0 and "nerf_hashgrid_forward" in msg, (what, rc, msg)
        rc = lib.nerf_hashgrid_backward(xw.data_ptr(), cs.emb.data_ptr(), go.data_ptr(), B, D, C, Lv, off, sc, ge.data_ptr(),
                                        out.data_ptr(), st)
        msg = lib.nerf_last_error().decode()
        assert rc != 0 and "nerf_hashgrid_backward" in msg, (what, rc, msg)
    assert (B31 - 1) * cs.L * cs.C < 1 << 31                               # (the largest B below it would have been accepted)
    # a level without rows, a misaligned table
    flat = (ctypes.c_int32 * (cs.L + 1))(*([0, 8, 8, 16, 24][:cs.L + 1]))
    assert lib.nerf_hashgrid_forward(x.data_ptr(), cs.emb.data_ptr(), 4, cs.D, cs.C, cs.L, flat, cs.sc_c, out.data_ptr(), st) != 0
    assert "offsets" in lib.nerf_last_error().decode()
    assert lib.nerf_hashgrid_forward(x.data_ptr(), cs.emb.data_ptr() + 4, 4, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c, out.data_ptr(), st) != 0
    assert "aligned" in lib.nerf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all()) and bool((ge == 0).all()) and _intact(we, cs.emb.numel())   # nothing was launched
    with pytest.raises(L.NerfLibraryError):
        L.check(lib.nerf_hashgrid_forward(x.data_ptr(), cs.emb.data_ptr(), 4, 5, cs.C, cs.L, cs.off_c, cs.sc_c, out.data_ptr(), st), "fwd")
