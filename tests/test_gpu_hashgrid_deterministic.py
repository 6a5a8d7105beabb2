"""GPU tests of the deterministic hash-grid table gradient (csrc/nerf_hashgrid_det.hip.inc, include/nerf_mi355x_hashgrid.h, DESIGN.md
section 2.12.1) against the integer restatement in tests/hashgrid_exact_reference.py, on configurations of tests/test_gpu_hashgrid.py.

What is asserted, and where the bounds come from:
  bits           grad_emb equals the restatement in every bit, into a buffer pre-filled with non-zero values (and some -0.0): elements
                 no live term reaches keep their bits, the others are fadd(previous, v).  The restatement sums integers, so there
                 is one right answer.
  order          the same bytes after a permutation of the points, and from two calls into equal buffers.
  exactness      1 + 2^-30 - 1 into one element is exactly 2^-30, in every order (fp32 atomics give 0 in two of three orders).
  poison         one Inf in grad_out: quiet NaN in exactly the elements its terms reach, the restatement's value everywhere else.
  accuracy       |got - truth| <= (2D + 2) * 2^-24 * sum|term| + k * 2^(emax - 150 - K) + 2^-24 * |truth| per element: the roundings
                 inside a term (D of 1 - f, D - 1 multiplies, the product with grad_out: 2D <= 2D + 2, as tests/test_gpu_hashgrid.py
                 counts them), one truncation below the unit 2^(emax - 150 - K) per term, and the single final rounding.  No term for
                 the order of summation: there is none.
  module         the input gradient does not depend on the flag; hash_encode, HashEncoder, TriPlane and HashField.density with the
                 flag give the bytes of the direct call; 30 Adam steps of an encoder run twice give equal tables and loss histories.
Every buffer the kernels write is the interior of a larger sentinel-filled one, the workspace included."""
import ctypes
import types

import pytest
import torch

import hashgrid_exact_reference as X
import hashgrid_reference as R
import test_gpu_hashgrid as G
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAMES = ("default", "dense_then_hashed", "d4_contended", "c1", "c8")
BATCHES = G.BATCHES
WS_SENTINEL, WS_PAD = 0xA5, 256     # WS_PAD bytes on each side: the interior keeps the 16-byte alignment the entry asks for
assert BATCHES == (1, 63, 64, 65, 513, 4096)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _workspace(amd, cs):
    need = amd._lib.call("nerf_hashgrid_deterministic_workspace_bytes", cs.off[-1] - cs.off[0], cs.C)
    assert need == X.workspace_bytes(cs.off[-1] - cs.off[0], cs.C)
    whole = torch.full((need + 2 * WS_PAD,), WS_SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[WS_PAD:WS_PAD + need], need


def _ws_intact(whole, need):
    return bool((whole[:WS_PAD] == WS_SENTINEL).all() and (whole[WS_PAD + need:] == WS_SENTINEL).all())


def _det(amd, cs, x, go, prev=None):
    """The direct call -> grad_emb [rows, C]; `prev`: what the buffer holds before (default zeros)."""
    B, ne = x.shape[0], cs.off[-1] * cs.C
    we, ge = G._padded(ne, zero=True)
    if prev is not None:
        ge.copy_(prev.reshape(-1))
    ws_whole, ws, need = _workspace(amd, cs)
    amd._lib.call("nerf_hashgrid_backward_deterministic", x, go, B, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c, ge, ws, need)
    torch.cuda.synchronize()
    assert G._intact(we, ne) and _ws_intact(ws_whole, need)
    return ge.view(cs.off[-1], cs.C)


_exact_cache = {}


def _exact(amd, name, B):
    """The restatement of configuration `name` at batch B into a zeroed table, computed once per module: x, go (GPU) and the result."""
    if (name, B) not in _exact_cache:
        cs = G.Case.get(name)
        x, go = cs.inputs(B)
        K = amd._lib.call("nerf_hashgrid_deterministic_guard_bits", B, cs.D)
        assert K == X.guard_bits(B, cs.D)
        _exact_cache[name, B] = (x, go, K, X.exact_table_gradient(x, cs.off, cs.sc, go, cs.C, K))
    return _exact_cache[name, B]


def _into(res, prev):
    """What the entry leaves in a buffer that held `prev` (CPU float32 [rows, C]): one fadd where a live term arrived."""
    emax = torch.from_numpy(res["emax"])
    want = torch.where(emax > 0, prev + res["grad"], prev)                 # (res["grad"] is the sum itself, or NaN where poisoned)
    want.view(torch.int32)[emax == 255] = X.QNAN_BITS
    return want


def _prefill(cs, seed):
    prev = torch.randn(cs.off[-1], cs.C, generator=torch.Generator().manual_seed(seed))
    prev.view(-1)[::7] = -0.0
    return prev


# ---- the direct call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bit_equal_to_the_restatement(amd, name):
    cs = G.Case.get(name)
    for B in BATCHES:
        x, go, K, res = _exact(amd, name, B)
        prev = _prefill(cs, B)
        got = _det(amd, cs, x, go, prev=prev.cuda()).cpu()
        want = _into(res, prev)
        same = _bits(got) == _bits(want)
        untouched = torch.from_numpy(res["emax"] == 0)
        print(f"    {name} B={B} K={K}: {int((~same).sum())} of {same.numel()} differ; {int((~untouched).sum())} elements touched")
        assert bool(same.all())
        assert torch.equal(_bits(got)[untouched], _bits(prev)[untouched])   # not read, not written: -0.0 stays -0.0
        assert bool((~untouched).any()) and bool((got != prev)[~untouched].any())
        # into a zeroed buffer: the sum itself
        assert torch.equal(_bits(_det(amd, cs, x, go).cpu()), _bits(res["grad"]))


@pytest.mark.parametrize("name", NAMES)
def test_order_independence(amd, name):
    cs = G.Case.get(name)
    for B in (65, 4096):
        x, go, _, res = _exact(amd, name, B)
        first = _det(amd, cs, x, go)
        assert torch.equal(_bits(first), _bits(_det(amd, cs, x, go)))       # run to run
        for seed in (1, 2):
            perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed)).cuda()
            assert torch.equal(_bits(first), _bits(_det(amd, cs, x[perm].contiguous(), go[perm].contiguous()))), (B, seed)
        assert torch.equal(_bits(first.cpu()), _bits(res["grad"]))


def test_a_level_table_that_does_not_start_at_row_zero(amd):
    """offsets[0] = 8: the workspace covers offsets[L] - offsets[0] rows, the rows before the first level are not touched."""
    base = G.Case.get("c8")
    off = [o + 8 for o in base.off]
    cs = types.SimpleNamespace(D=base.D, L=base.L, C=base.C, off=off, sc=base.sc, sc_c=base.sc_c,
                               off_c=(ctypes.c_int32 * (base.L + 1))(*off))
    x, go = base.inputs(65)
    prev = _prefill(cs, 1)
    got = _det(amd, cs, x, go, prev=prev.cuda()).cpu()
    res = X.exact_table_gradient(x, off, cs.sc, go, cs.C, X.guard_bits(65, cs.D), prev=prev)
    assert torch.equal(_bits(got), _bits(res["grad"])) and torch.equal(_bits(got[:8]), _bits(prev[:8]))
    assert (res["emax"][:8] == 0).all() and (res["emax"][8:] > 0).any()


def test_what_float_atomics_cannot_guarantee(amd):
    """Three identical points on a level-0 vertex (corner 0 weighs exactly 1, the other corners give null terms) with grad_out
    1, 2^-30, -1: the element is exactly 2^-30 in every order of the rows."""
    cs = G.Case.get("dense_then_hashed")
    xb = float(R.boundary_points(cs.H)[0])
    x = torch.full((3, cs.D), xb, device="cuda")
    go = torch.tensor([1.0, 2.0 ** -30, -1.0], device="cuda")[:, None].expand(3, cs.L * cs.C).contiguous()
    g, f = R.cells(x.cpu(), cs.sc[0])
    assert float(f.abs().max()) == 0.0
    row = int(R.corner_rows(g, 0, cs.off[1] - cs.off[0], cs.sc[0])[0])
    assert amd._lib.call("nerf_hashgrid_deterministic_guard_bits", 3, cs.D) == 30
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [0, 2, 1]):
        got = _det(amd, cs, x[order].contiguous(), go[order].contiguous()).cpu()
        assert bool((got[row] == 2.0 ** -30).all()), (order, got[row])
        rest = got[:cs.off[1]].clone()
        rest[row] = 0
        assert float(rest.abs().max()) == 0.0                              # the null terms of the other corners left nothing
        assert torch.equal(_bits(got), _bits(X.exact_table_gradient(x[order], cs.off, cs.sc, go[order], cs.C, 30)["grad"]))


@pytest.mark.parametrize("name", ["default", "d4_contended"])
def test_poison(amd, name):
    cs = G.Case.get(name)
    B = 65
    x, go, K, clean = _exact(amd, name, B)
    bad = go.clone()
    bad[40, 1 * cs.C] = float("inf")                                       # one channel of level 1 of one point
    res = X.exact_table_gradient(x, cs.off, cs.sc, bad, cs.C, K)
    prev = _prefill(cs, 3)
    got = _det(amd, cs, x, bad, prev=prev.cuda()).cpu()
    nan = torch.from_numpy(res["emax"] == 255)
    assert 1 <= int(nan.sum()) <= 2 ** cs.D and not bool(nan[:cs.off[1]].any()) and not bool(nan[cs.off[2]:].any())
    assert torch.equal(torch.isnan(got), nan) and bool((_bits(got)[nan] == X.QNAN_BITS).all())
    assert torch.equal(_bits(got), _bits(_into(res, prev)))
    assert torch.equal(_bits(got)[~nan], _bits(_into(clean, prev))[~nan])  # the other elements: as without the Inf


@pytest.mark.parametrize("name", NAMES)
def test_accuracy_within_the_derived_bound(amd, name):
    cs = G.Case.get(name)
    for B in BATCHES:
        x, go, K, res = _exact(amd, name, B)
        t = R.truth_f64(x, cs.emb, cs.off, cs.sc, go)
        truth, k = t["grad_emb"].cpu(), t["grad_emb_count"].cpu()
        got = _det(amd, cs, x, go).cpu()
        err = (got.double() - truth).abs()
        bound = (2 * cs.D + 2) * U * t["grad_emb_abs"].cpu() + torch.from_numpy(X.truncation_bound(k.numpy(), res["emax"], K)) + U * truth.abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"    {name} B={B} K={K}: max err / bound = {ratio:.3f}, max err {float(err.max()):.3e}")
        assert bool((err <= bound).all()), f"error above the bound (worst ratio {ratio:.3f})"
        assert bool((got[k == 0] == 0).all()) and float(got.abs().max()) > 0


def test_refusals_write_nothing(amd):
    L = amd._lib
    lib = L.load()
    cs = G.Case.get("dense_then_hashed")
    x, go = cs.inputs(65)
    ne = cs.off[-1] * cs.C
    we, ge = G._padded(ne, zero=True)
    ws_whole, ws, need = _workspace(amd, cs)
    st = L.stream_of(x.device)

    def call(ge_p=ge.data_ptr(), ws_p=ws.data_ptr(), nbytes=need, go_p=go.data_ptr(), B=65):
        rc = lib.nerf_hashgrid_backward_deterministic(x.data_ptr(), go_p, B, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c, ge_p, ws_p, nbytes, st)
        assert rc != 0 and "nerf_hashgrid_backward_deterministic" in lib.nerf_last_error().decode()
        return rc
    assert call(ws_p=None) == -1 and call(ge_p=None) == -1 and call(go_p=None) == -1
    assert call(ws_p=ws.data_ptr() + 8) == -1 and call(ge_p=ge.data_ptr() + 2) == -1 and call(go_p=go.data_ptr() + 4) == -1
    assert call(nbytes=need - 1) == -2 and call(nbytes=12 * ne - 1) == -2 and call(nbytes=0) == -2
    assert call(B=0) == -1
    torch.cuda.synchronize()
    assert bool((ge == 0).all()) and G._intact(we, ne)
    assert bool((ws_whole == WS_SENTINEL).all())                           # not even the zero-fill ran
    with pytest.raises(L.NerfLibraryError):
        L.call("nerf_hashgrid_backward_deterministic", x, go, 65, cs.D, cs.C, cs.L, cs.off_c, cs.sc_c, ge, ws[:need - 256], need - 256)
    torch.cuda.synchronize()
    assert bool((ge == 0).all()) and bool((ws_whole == WS_SENTINEL).all())


# ---- the module ------------------------------------------------------------------------------------------------------------------------
def _encoder(amd, cs, deterministic):
    enc = amd.HashEncoder(input_dim=cs.D, num_levels=cs.L, level_dim=cs.C, per_level_scale=cs.s, base_resolution=cs.H,
                          log2_hashmap_size=cs.T, deterministic=deterministic).cuda()
    assert enc.offsets.tolist() == cs.off and enc.deterministic is deterministic
    with torch.no_grad():
        enc.embeddings.copy_(cs.emb)
    return enc


@pytest.mark.parametrize("name", ["dense_then_hashed", "c8"])
def test_autograd_equals_the_direct_calls(amd, name):
    from nerf_replication_amd.hashgrid import hash_encode
    cs = G.Case.get(name)
    x, go = cs.inputs(513)
    direct = _det(amd, cs, x, go)
    _, gx_direct, _ = G._backward(amd, cs, x, go, want_emb=False)
    # hash_encode: both gradients, the table gradient alone, and the flag off
    emb = cs.emb.clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    out = hash_encode(xr, emb, cs.off, cs.s, cs.H, deterministic=True)
    assert torch.equal(out.detach(), G._forward(amd, cs, x))
    gx, ge = torch.autograd.grad(out, (xr, emb), go)
    assert torch.equal(_bits(ge), _bits(direct)) and torch.equal(gx, gx_direct)
    (ge,) = torch.autograd.grad(hash_encode(x, emb, cs.off, cs.s, cs.H, deterministic=True), (emb,), go)
    assert torch.equal(_bits(ge), _bits(direct))
    out = hash_encode(xr, emb, cs.off, cs.s, cs.H)
    gx_off, ge_off = torch.autograd.grad(out, (xr, emb), go)
    assert torch.equal(gx_off, gx)                                         # the input gradient: bit-equal with the flag on and off
    assert float((ge_off - direct).abs().max()) <= 1e-4 * float(direct.abs().max())      # (the atomics path, within its own error)
    # a frozen table with the flag: the input gradient alone
    (gx_only,) = torch.autograd.grad(hash_encode(xr, cs.emb, cs.off, cs.s, cs.H, deterministic=True), (xr,), go)
    assert torch.equal(gx_only, gx_direct)
    # HashEncoder, prefix shape [19, 27, D]; the attribute may be flipped between steps
    enc = _encoder(amd, cs, True)
    xp = x.view(19, 27, cs.D).clone().requires_grad_(True)
    gx, ge = torch.autograd.grad(enc(xp, normalize=False), (xp, enc.embeddings), go.view(19, 27, -1))
    assert torch.equal(_bits(ge), _bits(direct)) and torch.equal(gx.view(513, cs.D), gx_direct)
    enc.deterministic = False
    (ge_off2,) = torch.autograd.grad(enc(x, normalize=False), (enc.embeddings,), go)
    assert float((ge_off2 - direct).abs().max()) <= 1e-4 * float(direct.abs().max())
    # a table with rows beyond the level table: they get exact zeros
    wide = torch.cat([cs.emb, torch.ones(5, cs.C, device="cuda")]).requires_grad_(True)
    (ge,) = torch.autograd.grad(hash_encode(x, wide, cs.off, cs.s, cs.H, deterministic=True), (wide,), go)
    assert torch.equal(_bits(ge[:-5]), _bits(direct)) and bool((ge[-5:] == 0).all())


def test_triplane_planes_get_the_direct_call(amd):
    tri = amd.TriPlane(num_levels=4, level_dim=2, base_resolution=15, log2_hashmap_size=10, deterministic=True).cuda()
    wb = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], device="cuda")
    with torch.no_grad():
        for p in tri.parameters():
            p.uniform_(-1, 1)
    gen = torch.Generator(device="cuda").manual_seed(2)
    xyz = torch.rand(2, 33, 3, device="cuda", generator=gen)
    go = torch.randn(2, 33, tri.out_dim, device="cuda", generator=gen)
    tri(xyz, wb).backward(go)
    norm = (torch.clamp(xyz, min=wb[:3], max=wb[3:]) - wb[:3]) / (1.0 + 1e-6)
    off, sc = R.level_offsets(2, 4, 2, 15, 10), R.level_scales(4, 2, 15)
    cs = types.SimpleNamespace(D=2, L=4, C=2, off=off, sc=sc, off_c=(ctypes.c_int32 * 5)(*off), sc_c=(ctypes.c_float * 4)(*[float(v) for v in sc]))
    for i, (plane, ax) in enumerate(((tri.xy_plane, [0, 1]), (tri.yz_plane, [1, 2]), (tri.xz_plane, [0, 2]))):
        assert plane.deterministic is True
        direct = _det(amd, cs, norm[..., ax].reshape(-1, 2).contiguous(), go.view(66, -1)[:, 8 * i:8 * i + 8].contiguous())
        assert torch.equal(_bits(plane.embeddings.grad), _bits(direct)) and float(direct.abs().max()) > 0


def test_hashfield_density_hands_the_flag_on(amd, monkeypatch):
    from nerf_replication_amd import hashfield
    cs = G.Case.get("dense_then_hashed")
    seen = []
    real = hashfield.hash_encode

    def spy(inputs, embeddings, offsets, s, H, deterministic=False):
        out = real(inputs, embeddings, offsets, s, H, deterministic)
        seen.append([deterministic, inputs.detach().clone(), None])
        out.register_hook(lambda g, rec=seen[-1]: rec.__setitem__(2, g.detach().clone()))
        return out
    monkeypatch.setattr(hashfield, "hash_encode", spy)
    torch.manual_seed(0)
    field = amd.HashField([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], encoder=_encoder(amd, cs, True)).cuda()
    xyz = (torch.rand(513, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) - 0.5) * 2.8
    grads = []
    for _ in range(2):
        field.zero_grad(set_to_none=True)
        field.density(xyz).sum().backward()
        grads.append(field.encoder.embeddings.grad.clone())
    assert torch.equal(_bits(grads[0]), _bits(grads[1])) and float(grads[0].abs().max()) > 0
    assert [s[0] for s in seen] == [True, True]
    direct = _det(amd, cs, seen[0][1].contiguous(), seen[0][2].contiguous())
    assert torch.equal(_bits(grads[0]), _bits(direct))


def test_training_an_encoder_twice_gives_the_same_bytes(amd):
    """30 Adam steps, T = 12, B = 4096; the loss is elementwise operations and sum (no GEMM: its order is not ours to promise)."""
    cs = G.Case.get("dense_then_hashed")
    assert cs.T == 12
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(4096, cs.D, device="cuda", generator=gen)
    target = torch.sin(6.0 * x.sum(dim=1, keepdim=True) + torch.arange(cs.L * cs.C, device="cuda")[None]) * 0.5

    def run():
        torch.manual_seed(3)
        enc = amd.HashEncoder(input_dim=cs.D, num_levels=cs.L, level_dim=cs.C, per_level_scale=cs.s, base_resolution=cs.H,
                              log2_hashmap_size=cs.T, deterministic=True).cuda()
        opt = torch.optim.Adam(enc.parameters(), lr=1e-2)
        losses = []
        for _ in range(30):
            opt.zero_grad(set_to_none=True)
            diff = enc(x, normalize=False) - target
            loss = (diff * diff).sum()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        return enc.embeddings.detach().clone(), torch.stack(losses)
    emb_a, loss_a = run()
    emb_b, loss_b = run()
    print(f"    loss {float(loss_a[0]):.4f} -> {float(loss_a[-1]):.4f}")
    assert torch.equal(_bits(emb_a), _bits(emb_b)) and torch.equal(_bits(loss_a), _bits(loss_b))
    assert float(loss_a[-1]) < float(loss_a[0]) and bool(torch.isfinite(loss_a).all())
