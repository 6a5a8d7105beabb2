"""GPU checks of the deformation field: nerf_deform_forward bit for bit against the fp32 restatement
(tests/deform_reference.py), the pack round trip, the table gradient against float64 by the rule of DESIGN.md section 2.13
    max|hip - f64| <= 3 max|cpu_fp32 - f64| + 2 u max|f64|        (both sides from the restatement, never from the code under test)
and a dynamic HashField (encoder = DNeRFNGP) against the restatement of the whole path: render, every parameter gradient, the
canonical frame, chunking, importance sampling with jitter stage by stage, density at a frame, training."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import deform_reference as DR
import hashfield_reference as R
import hashfield_sampling_reference as SR
import hashgrid_reference as H
from gpu_common import amd  # noqa: F401  (fixture)
from test_gpu_hashfield import Guarded, SENTINEL, _allowed, same

pytestmark = pytest.mark.gpu

U = R.U
DEFORM_JSON = os.path.join(R.REPO, "profiles", "deform_parity.json")
SHAPES = [(2, 2), (3, 5), (5, 8)]
ROWS = [1, 63, 65, 257]
S_KERNEL = 3                                          # samples per ray of the kernel-level cases: a ray's time serves three rows


def times_of(n_rays, T, gen):
    """Frame numbers per ray: 0 (canonical), an integer, T - 1, fractional, below 0, above T - 1, -0, then random ones."""
    t = torch.rand(n_rays, generator=gen) * (T - 1)
    special = [0.0, float(min(1, T - 1)), float(T - 1), 0.37 * (T - 1), -2.5, T + 3.0, -0.0]
    for k, v in enumerate(special):                                # every eighth ray keeps its random time
        t[k::8] = v
    if n_rays == 1:
        t[0] = 0.37 * (T - 1)
    return t.contiguous()


@functools.lru_cache(maxsize=None)
def kernel_case(n_rows, T, Rr, with_index):
    """Inputs and the restatement's outputs of one kernel-level case, computed once.  The clamp of x + delta is active on some rows
    and inactive on others, and (asserted on the float64 side) no live coordinate lies within 1e-4 of its boundary: coordinates that
    do are redrawn."""
    gen = torch.Generator().manual_seed(1000 * n_rows + 10 * T + Rr + int(with_index))
    feat = [(0.4 * torch.randn(3, 64, T, Rr, generator=gen)).numpy() for _ in range(3)]
    n_rays = n_rows if with_index else (n_rows + S_KERNEL - 1) // S_KERNEL
    P = n_rays * S_KERNEL
    index = None
    if with_index:                                    # ascending, with gaps; the last id is out of range when there is another row
        index = torch.sort(torch.randperm(P, generator=gen)[:n_rows]).values.to(torch.int32)
        if n_rows > 1:
            index[-1] = P + 5
    ids = R.ids_of(index, n_rows)
    live = (ids >= 0) & (ids < P)
    time = times_of(n_rays, T, gen)
    t_rows = time[torch.clamp(ids, 0, P - 1) // S_KERNEL].numpy()
    x = torch.rand(n_rows, 3, generator=gen)
    x[0, 0] = 0.0                                     # a coordinate exactly 0 and one exactly 1
    x[n_rows // 2, 1] = 1.0
    if n_rows > 2:
        x[2] = torch.tensor([1.0, 0.0, 1.0])
    x = x.numpy()
    for _ in range(20):
        s, _ = DR.gate(x, t_rows, feat)
        near = (np.abs(s) < 1e-4) | (np.abs(s - 1) < 1e-4)
        if not near.any():
            break
        x = np.where(near, torch.rand(n_rows, 3, generator=gen).numpy(), x).astype(np.float32)
    s, open_ = DR.gate(x, t_rows, feat)
    assert not ((np.abs(s) < 1e-4) | (np.abs(s - 1) < 1e-4)).any()
    g = torch.randn(n_rows, 3, generator=gen).numpy()
    delta, warped = DR.deform(x, t_rows, feat, np.float32)
    lv = live.numpy()
    grads = {}
    for tag, dtype in (("f64", np.float64), ("cpu32", np.float32)):
        grads[tag] = DR.table_gradient(x[lv], t_rows[lv], feat, g_x_warped=g[lv], dtype=dtype)
    return {"feat": feat, "n_rays": n_rays, "index": index, "live": lv, "time": time, "t_rows": t_rows, "x": x, "g": g,
            "delta": delta, "warped": warped, "open": open_, "grads": grads}


def device_tables(amd, feat, T, Rr):
    """(the three tables on the device, packed) through nerf_deform_pack, the packed buffer guarded."""
    tabs = [torch.from_numpy(f).cuda().contiguous() for f in feat]
    nbytes = amd._lib.call("nerf_deform_packed_bytes", 64, T, Rr)
    assert nbytes == 9 * T * Rr * 64 * 4 and amd._lib.call("nerf_deform_table_bytes", 64, T, Rr) == tabs[0].numel() * 4
    packed = Guarded((nbytes // 4,))
    assert packed.view.data_ptr() % 256 == 0
    amd._lib.call("nerf_deform_pack", tabs, 64, T, Rr, packed.view)
    return tabs, packed


# ---- the entries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Rr", SHAPES)
def test_pack_round_trip(amd, T, Rr):
    gen = torch.Generator().manual_seed(T * 100 + Rr)
    feat = [torch.randn(3, 64, T, Rr, generator=gen).numpy() for _ in range(3)]
    tabs, packed = device_tables(amd, feat, T, Rr)
    assert same(packed.view, torch.from_numpy(DR.pack(feat)), "packed") and packed.intact()
    got = packed.view.cpu().numpy()                                # the header's index function, element by element
    for i, j, y, c, f in [(0, 0, 0, 0, 0), (2, 2, T - 1, Rr - 1, 63), (1, 2, 1, Rr // 2, 17), (2, 0, T - 1, 0, 40), (0, 1, 0, Rr - 1, 1)]:
        assert got[DR.packed_index(i, j, y, c, f, T, Rr)] == feat[i][j, f, y, c]
    back = [Guarded((3, 64, T, Rr)) for _ in range(3)]
    amd._lib.call("nerf_deform_unpack_grad", packed.view, 64, T, Rr, [b.view for b in back])
    for i in range(3):
        assert same(back[i].view, torch.from_numpy(feat[i]), f"table {i}") and back[i].intact()


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("T,Rr", SHAPES)
@pytest.mark.parametrize("n_rows", ROWS)
def test_forward_is_the_restatement(amd, n_rows, T, Rr, with_index):
    c = kernel_case(n_rows, T, Rr, with_index)
    live, t_rows = c["live"], c["t_rows"]
    canon = live & (t_rows == 0)
    moved = live & (t_rows != 0)
    if n_rows >= 63:                                               # the cases hold what they are meant to hold
        assert canon.any() and (t_rows[live] < 0).any() and (t_rows[live] > T - 1).any() and (t_rows[live] == T - 1).any()
        assert ((c["warped"][moved] == 0) | (c["warped"][moved] == 1)).any() and c["open"][moved].any()
        assert (c["x"][live] == 0).any() and (c["x"][live] == 1).any()
    _, packed = device_tables(amd, c["feat"], T, Rr)
    xg, tg = torch.from_numpy(c["x"]).cuda(), c["time"].cuda()
    ig = None if c["index"] is None else c["index"].cuda()
    want_w = torch.from_numpy(np.where(live[:, None], c["warped"], np.float32(SENTINEL)))     # a skipped row is not written
    want_d = torch.from_numpy(np.where(live[:, None], c["delta"], np.float32(SENTINEL)))
    for outputs in ("both", "warped", "delta"):
        xw = Guarded((n_rows, 3), fill=SENTINEL) if outputs != "delta" else None
        dl = Guarded((n_rows, 3), fill=SENTINEL) if outputs != "warped" else None
        amd._lib.call("nerf_deform_forward", xg, tg, ig, n_rows, c["n_rays"], S_KERNEL, packed.view, 64, T, Rr,
                      None if xw is None else xw.view, None if dl is None else dl.view)
        if xw is not None:
            assert same(xw.view, want_w, "x_warped") and xw.intact(), outputs
            got = xw.view.cpu().numpy()
            assert np.array_equal(got[canon].view(np.int32), c["x"][canon].view(np.int32))     # the canonical frame: x's bits
        if dl is not None:
            assert same(dl.view, want_d, "delta") and dl.intact(), outputs
    assert packed.intact()


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("T,Rr", SHAPES)
@pytest.mark.parametrize("n_rows", ROWS)
def test_table_gradient(amd, n_rows, T, Rr, with_index):
    """The rule of the module's docstring per tensor, the CPU side summing the rows in their order.  The device adds with fp32
    atomics whose order changes from run to run, so its distance from float64 is a different figure every run.  Measured over 40
    launches, as a fraction of the allowance (worst tensor): 257 rows, (5, 8), no index: 0.30-0.35; 257 rows, (2, 2), index:
    0.23-0.48; 257 rows, (2, 2), no index -- every row adds into the same four taps of every plane, 257 terms per element, and the
    CPU's one order happens to land 4.8e-7 from float64 where the device's orders land 0.9e-6..2.0e-6 -- 0.44-1.002, median 0.64:
    ONE LAUNCH IN 40 MISSED THE BOUND THERE, by 0.2 %.  The bound and the cases are the issue's and stay as they are."""
    c = kernel_case(n_rows, T, Rr, with_index)
    live, moved = c["live"], c["live"] & (c["t_rows"] != 0)
    if n_rows >= 63:
        assert c["open"][moved].any() and (~c["open"][moved]).any()                       # the clamp: active and inactive rows
    _, packed = device_tables(amd, c["feat"], T, Rr)
    xg, tg, gg = torch.from_numpy(c["x"]).cuda(), c["time"].cuda(), torch.from_numpy(c["g"]).cuda()
    ig = None if c["index"] is None else c["index"].cuda()
    g_packed = Guarded((9 * T * Rr * 64,), fill=0.0)
    amd._lib.call("nerf_deform_backward", xg, tg, ig, n_rows, c["n_rays"], S_KERNEL, packed.view, 64, T, Rr, gg, None, g_packed.view)
    grads = [Guarded((3, 64, T, Rr)) for _ in range(3)]
    amd._lib.call("nerf_deform_unpack_grad", g_packed.view, 64, T, Rr, [b.view for b in grads])
    assert g_packed.intact() and packed.intact() and all(b.intact() for b in grads)
    figures, ok = {}, []
    for i in range(3):
        hip, f64, c32 = grads[i].view.cpu(), torch.from_numpy(c["grads"]["f64"][i]), torch.from_numpy(c["grads"]["cpu32"][i])
        ok.append(_allowed(f"grad_feat{i}", hip, f64, c32, figures))
        # elements no live row reaches (canonical rays among them) and elements behind an inactive clamp: exactly zero
        assert bool((hip[f64 == 0] == 0).all()), i
        if moved.any() and c["open"][moved][:, i].any():
            assert float(f64.abs().max()) > 0
    all_figures = dict(figures)
    assert all(ok), figures
    # the gradient of delta is not gated and reaches frame 0: canonical rows count, a NaN time adds nothing
    t_nan = c["time"].clone()
    t_nan[-1] = float("nan")
    rows = c["t_rows"].copy()
    ids = R.ids_of(c["index"], n_rows)
    rows[(torch.clamp(ids, 0, c["n_rays"] * S_KERNEL - 1) // S_KERNEL == c["n_rays"] - 1).numpy()] = np.nan
    g_packed = Guarded((9 * T * Rr * 64,), fill=0.0)
    amd._lib.call("nerf_deform_backward", xg, t_nan.cuda(), ig, n_rows, c["n_rays"], S_KERNEL, packed.view, 64, T, Rr, None, gg,
                  g_packed.view)
    got = DR.unpack(g_packed.view.cpu().numpy(), T, Rr)
    figures, ok = {}, []
    for tag, dtype in (("f64", np.float64), ("cpu32", np.float32)):
        c["grads"][tag + "_delta"] = DR.table_gradient(c["x"][live], rows[live], c["feat"], g_delta=c["g"][live], dtype=dtype)
    for i in range(3):
        f64 = torch.from_numpy(c["grads"]["f64_delta"][i])
        ok.append(_allowed(f"grad_delta_feat{i}", torch.from_numpy(got[i]), f64, torch.from_numpy(c["grads"]["cpu32_delta"][i]), figures))
        assert bool((torch.from_numpy(got[i])[f64 == 0] == 0).all()), i
    all_figures.update(figures)
    record(f"kernel_rows{n_rows}_T{T}_R{Rr}_{'index' if with_index else 'all'}", all_figures)
    assert all(ok), figures


# ---- the module ------------------------------------------------------------------------------------------------------------------------
ENC = dict(input_dim=3, num_levels=4, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=12)


def test_module_against_the_reference_project(amd):
    """DNeRFNGP.compute_delta and its gradient on the golden inputs: the reference's own float64 run is the yardstick, the fp32
    restatement the CPU side of the rule.  The packed copy is made once and remade when a table is written."""
    z = np.load(os.path.join(R.REPO, "tests", "golden", "deform_delta.npz"))
    feat = [z[f"feat{i}"] for i in range(3)]
    m = amd.DNeRFNGP(5, reso=8, **ENC)
    m.load_state_dict({"encoder.embeddings": m.encoder.embeddings.detach(), **{f"feat.{i}": torch.from_numpy(feat[i]) for i in range(3)}})
    m = m.cuda()
    x, t, g = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["t"]).cuda()[:, None], torch.from_numpy(z["g"]).cuda()
    with torch.no_grad():
        d0 = m.compute_delta(x, t)
        packed = m.packed()
        assert m.packed() is packed and not d0.requires_grad                      # inference packs once
    delta = m.compute_delta(x, t)
    want, _ = DR.deform(z["x"], z["t"], feat, np.float32)
    assert same(delta, torch.from_numpy(want), "delta") and torch.equal(d0, delta.detach())
    assert same(m.compute_delta(x.view(1, 257, 3), t.view(1, 257, 1)).view(257, 3), torch.from_numpy(want), "delta [1,N,3]")
    (delta * g).sum().backward()
    c32 = DR.table_gradient(z["x"], z["t"], feat, g_delta=z["g"], dtype=np.float32)
    figures = {}
    ok = [_allowed(f"grad_feat{i}", m.feat[i].grad, torch.from_numpy(z[f"grad{i}"]), torch.from_numpy(c32[i]), figures) for i in range(3)]
    assert all(ok), figures
    assert m.encoder.embeddings.grad is None
    with pytest.raises(RuntimeError):                                             # once differentiable
        d = m.compute_delta(x, t)
        gr, = torch.autograd.grad((d * g).sum(), m.feat[0], create_graph=True)
        gr.sum().backward()
    with torch.no_grad():
        m.feat[0].mul_(2.0)
    assert m.packed() is not packed                                               # a written table is packed again
    # forward: normalise, warp, encode; a point at frame 0 is encoded where it is
    wb = torch.tensor(R.BBOX, dtype=torch.float32).cuda()
    xyz = (torch.rand(64, 3, generator=torch.Generator().manual_seed(4)) * 3.4 - 1.7).cuda()
    tt = torch.full((64, 1), 2.5).cuda()
    tt[:8] = 0.0
    with torch.no_grad():
        out = m(torch.cat([xyz, tt], -1), wb)
        x01 = amd.hashgrid.normalize_to_bounds(xyz, wb)
        feat_now = [f.detach().cpu().numpy() for f in m.feat]
        _, xw = DR.deform(x01.cpu().numpy(), tt[:, 0].cpu().numpy(), feat_now, np.float32)
        assert torch.equal(out, m.encoder(torch.from_numpy(xw).cuda(), normalize=False)) and out.shape == (64, 8)
        assert torch.equal(out[:8], m.encoder(x01[:8], normalize=False))
        # the smoothness term: torch's expression on compute_delta
        tv = m.compute_tv_loss(xyz.view(2, 32, 3), tt.view(2, 32, 1) + 1.0, wb)
        d1, _ = DR.deform(x01.cpu().numpy(), tt[:, 0].cpu().numpy() + 1.0, feat_now, np.float32)
        d0_, _ = DR.deform(x01.cpu().numpy(), tt[:, 0].cpu().numpy(), feat_now, np.float32)
        want_tv = torch.from_numpy(d1 - d0_).view(2, 32, 3).pow(2).sum(dim=1).sum(dim=1, keepdim=True)
        assert tv.shape == (2, 1) and torch.allclose(tv.cpu(), want_tv, rtol=1e-5, atol=0)
        # a batch whose first frame number is 0: the squared offset itself, at frame 0 (delta is not the canonical identity)
        t0 = torch.zeros(2, 32, 1).cuda()
        tv0 = m.compute_tv_loss(xyz.view(2, 32, 3), t0, wb)
        dz, _ = DR.deform(x01.cpu().numpy(), np.zeros(64, dtype=np.float32), feat_now, np.float32)
        want_tv0 = torch.from_numpy(dz).view(2, 32, 3).pow(2).sum(dim=1).sum(dim=1, keepdim=True)
        assert tv0.shape == (2, 1) and float(want_tv0.min()) > 0 and torch.allclose(tv0.cpu(), want_tv0, rtol=1e-5, atol=0)


# ---- a dynamic field -------------------------------------------------------------------------------------------------------------------
T_FIELD, R_FIELD = 5, 8
PARAM_KEYS = ["encoder.encoder.embeddings"] + [f"encoder.feat.{i}" for i in range(3)] + \
             [f"sigma_net.layers.{i}.{p}" for i in range(2) for p in ("weight", "bias")] + \
             [f"color_net.layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")]


def field_tables(seed=21):
    """Tables whose warp moves a sample by about a cell of the finest level (1 / 128 of the box): 64 products of three bilinear
    values of N(0, 0.15^2) tables (test_field_render_and_gradients prints and bounds the mean step)."""
    gen = torch.Generator().manual_seed(seed)
    return [(0.15 * torch.randn(3, 64, T_FIELD, R_FIELD, generator=gen)).numpy() for _ in range(3)]


def ray_times(n, seed=5):
    gen = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=gen) * (T_FIELD - 1)
    t[0::7] = 0.0                                                                 # canonical rays
    t[1::7] = 2.0
    t[2::7] = float(T_FIELD - 1)
    return t.contiguous()


def dynamic_field(amd, sc, feat, requires_grad=True):
    enc = amd.DNeRFNGP(T_FIELD, reso=R_FIELD, input_dim=3, num_levels=sc["L"], level_dim=2, per_level_scale=2, base_resolution=16,
                       log2_hashmap_size=sc["T"])
    assert enc.encoder.offsets.tolist() == list(sc["offsets"])
    field = amd.HashField(R.BBOX, encoder=enc, width=sc["width"])
    flat = R.flat_params(sc["params"])
    values = [flat[0]] + [torch.from_numpy(f) for f in feat] + flat[1:]
    assert [k for k, _ in field.named_parameters()] == PARAM_KEYS and field.num_frames == T_FIELD
    with torch.no_grad():
        for p, v in zip(field.parameters(), values):
            assert p.shape == v.shape
            p.copy_(v)
    field = field.cuda()
    for p in field.parameters():
        p.requires_grad_(requires_grad)
    return field


def renderer_of(amd, field, S, white=True):
    ren = amd.HashRenderer(field)
    ren.N_samples, ren.white_bkgd = S, bool(white)
    return ren


def hash_forward_x(x32, x_live, emb, offsets, scales):
    """hashfield_reference.hash_forward that also carries the derivative with respect to the position: the cell and the fraction come
    from the float32 x32, x_live (emb's dtype, equal to x32) adds d pos / d x = scale (hashgrid_reference.forward_autograd_f64)."""
    B, D = x32.shape
    C, L = emb.shape[1], len(offsets) - 1
    outs = []
    for l in range(L):
        n = int(offsets[l + 1] - offsets[l])
        g, f32 = H.cells(x32, scales[l])
        f = f32.to(emb.dtype) + (x_live - x_live.detach()) * float(np.float32(scales[l]))
        omf = 1 - f
        acc = torch.zeros(B, C, dtype=emb.dtype)
        for idx in range(1 << D):
            acc = acc + H.corner_weight(f, idx, omf)[:, None] * emb[H.corner_rows(g, idx, n, scales[l]) + int(offsets[l])]
        outs.append(acc)
    return torch.cat(outs, dim=1)


def warp_rows(sc, feat, t, time):
    """(x32 [n*S,3] float32 before the warp, the warped positions float32, the frame number per row) on depths t [n,S]."""
    n, S = t.shape
    x32 = SR.points_rays(sc["o"], sc["d"], t, None, n * S, sc["frame"])
    t_rows = time.repeat_interleave(S).numpy()
    _, xw = DR.deform(x32.numpy(), t_rows, feat, np.float32)
    return x32, torch.from_numpy(xw), t_rows


def dynamic_render(sc, feat, t, time, white, dtype, grads=None):
    """The whole path of a dynamic field in `dtype` on depths t [n,S] (constants): the fp32 warped positions are the encoder's input
    in both dtypes, as the fp32 positions are for a static field.  grads = (a, b): also the gradients of sum(rgb a) + sum(depth b)
    with respect to every parameter, in PARAM_KEYS' order; the tables' come from the gradient that reaches the warped positions
    through deform_reference.table_gradient in the same dtype."""
    n, S = t.shape
    params = R.cast_params(sc["params"], dtype, requires_grad=grads is not None)
    x32, xw, t_rows = warp_rows(sc, feat, t, time)
    x_live = xw.to(dtype).clone().requires_grad_(grads is not None)          # (a copy: xw itself stays a constant)
    geo, _ = R.mlp(hash_forward_x(xw, x_live, params["emb"], sc["offsets"], sc["scales"]), params["sw"], params["sb"])
    sh = R.sh4(sc["d"], dtype)
    rgb_raw, _ = R.mlp(torch.cat([geo, sh.repeat_interleave(S, dim=0)], dim=1), params["cw"], params["cb"])
    raw = torch.cat([rgb_raw, geo[:, :1]], dim=1).view(n, S, 4)
    rgb, depth, weights = SR.composite_rays(raw, t, white, dtype)
    if grads is None:
        return rgb.detach(), depth.detach(), weights.detach(), geo[:, 0].detach()
    a, b = grads
    ((rgb * a.to(dtype)).sum() + (depth * b.to(dtype)).sum()).backward()
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    g_feat = DR.table_gradient(x32.numpy(), t_rows, feat, g_x_warped=x_live.grad.numpy(), dtype=np_dtype)
    flat = [p.grad for p in R.flat_params(params)]
    return rgb.detach(), depth.detach(), [flat[0]] + [torch.from_numpy(g) for g in g_feat] + flat[1:]


@functools.lru_cache(maxsize=None)
def field_reference(S, white, with_grads):
    sc = R.scene(65, S)
    feat, time = field_tables(), ray_times(65)
    t = sc["t"][None].expand(65, S).contiguous()
    gen = torch.Generator().manual_seed(77)
    a, b = torch.randn(65, 3, generator=gen), torch.randn(65, generator=gen)
    out = {"scene": sc, "feat": feat, "time": time, "a": a, "b": b}
    x32, xw, t_rows = warp_rows(sc, feat, t, time)
    s, open_ = DR.gate(x32.numpy(), t_rows, feat)
    moved = t_rows != 0
    out["moved_cells"] = float(np.abs(xw.numpy() - x32.numpy())[moved].mean() * 128)
    out["boundary"] = float(np.minimum(np.abs(s), np.abs(s - 1))[moved].min())
    out["open"] = float(open_[moved].mean())
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        out[tag] = dynamic_render(sc, feat, t, time, white, dtype, (a, b) if with_grads else None)
    return out


def batch_of(sc, time):
    return {"rays_o": sc["o"].cuda()[None], "rays_d": sc["d"].cuda()[None], "time": time.cuda()[None]}


def record(key, stats):
    rec = {}
    if os.path.exists(DEFORM_JSON):
        with open(DEFORM_JSON) as f:
            rec = json.load(f)
    rec[key] = stats
    with open(DEFORM_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("S", [64, 3])
def test_field_render_and_gradients(amd, S):
    ref = field_reference(S, 1, True)
    sc = ref["scene"]
    print(f"S={S}: the warp moves a sample by {ref['moved_cells']:.2f} finest cells on average; the clamp is open on "
          f"{ref['open']:.2f} of the coordinates, the nearest is {ref['boundary']:.2e} from its boundary")
    assert 0.3 < ref["moved_cells"] < 3.0 and 0.0 < ref["open"] < 1.0
    assert ref["boundary"] > 1e-6                                  # the gate decides the same way in fp32 and in float64
    assert float(ref["f64"][0].std()) > 1e-3
    ren = renderer_of(amd, dynamic_field(amd, sc, ref["feat"]), S)
    rgb, depth = ren.render(batch_of(sc, ref["time"]))
    assert rgb.shape == (65, 3) and depth.shape == (65,) and rgb.requires_grad
    ((rgb * ref["a"].cuda()).sum() + (depth * ref["b"].cuda()).sum()).backward()
    figures = {}
    ok = [_allowed("rgb", rgb, ref["f64"][0], ref["cpu32"][0], figures), _allowed("depth", depth, ref["f64"][1], ref["cpu32"][1], figures)]
    for name, p, g64, g32 in zip(PARAM_KEYS, ren.field.parameters(), ref["f64"][2], ref["cpu32"][2]):
        assert p.grad is not None and p.grad.shape == g64.shape and float(g64.abs().max()) > 0, name
        ok.append(_allowed("grad_" + name, p.grad, g64, g32, figures))
        if "feat" in name:                                          # table elements that nothing reaches: exactly zero
            assert bool((p.grad.cpu()[g64 == 0] == 0).all()), name
    record(f"field_S{S}", figures)
    assert all(ok), [k for k, o in zip(figures, ok) if not o]
    with torch.no_grad():                                          # grad mode does not change the bytes
        again = ren.render(batch_of(sc, ref["time"]))
    assert torch.equal(again[0], rgb.detach()) and torch.equal(again[1], depth.detach())
    # time per image [B] and [B,1]: one frame for all rays
    one = ren.render({**batch_of(sc, ref["time"]), "time": torch.full((1,), 2.5).cuda()})
    col = ren.render({**batch_of(sc, ref["time"]), "time": torch.full((1, 1), 2.5).cuda()})
    per_ray = ren.render(batch_of(sc, torch.full((65,), 2.5)))
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(one, col, per_ray))
    assert not torch.equal(one[0], rgb.detach())


def test_canonical_frame_is_the_static_field(amd):
    """Every time 0: the bytes of the static field with the same encoder and heads, image and gradients of the shared parameters;
    the tables get a gradient of exactly zero."""
    sc = R.scene(65, 64)
    dyn = dynamic_field(amd, sc, field_tables())
    enc = amd.HashEncoder(input_dim=3, num_levels=sc["L"], level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=sc["T"])
    static = amd.HashField(R.BBOX, encoder=enc, width=sc["width"])
    with torch.no_grad():
        for p, v in zip(static.parameters(), R.flat_params(sc["params"])):
            p.copy_(v)
    static = static.cuda()
    assert static.num_frames is None
    batch = batch_of(sc, torch.zeros(65))
    with torch.no_grad():
        got = renderer_of(amd, dyn, 64).render(batch)
        want = renderer_of(amd, static, 64).render(batch)                         # a static field ignores the key
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and float(want[0].std()) > 1e-3
    rgb, _ = renderer_of(amd, dyn, 64).render(batch)
    rgb.square().sum().backward()
    assert all(bool((f.grad == 0).all()) for f in dyn.encoder.feat)
    assert float(dyn.encoder.encoder.embeddings.grad.abs().max()) > 0


def test_chunking_does_not_change_the_bytes(amd):
    sc = R.scene(100, 64)
    ren = renderer_of(amd, dynamic_field(amd, sc, field_tables(), requires_grad=False), 64)
    batch = batch_of(sc, ray_times(100))
    results = []
    for chunk in (100, 33, 1):
        ren.chunk_rays = chunk
        results.append(ren.render(batch))
    for rgb, depth in results[1:]:
        assert torch.equal(rgb, results[0][0]) and torch.equal(depth, results[0][1])
    assert results[0][0].shape == (100, 3)


def test_importance_sampling_with_jitter_stage_by_stage(amd):
    """N_importance 8 + 8 with perturb: the jittered depths and the sampler bit for bit on the recorded draws and the device's own
    weights, the coarse weights and the image on the device's own depths by the rule (test_gpu_hashfield_sampling.py's decoupling)."""
    Sc, Sf = 8, 8
    sc = R.scene(65, Sc)
    feat, time = field_tables(), ray_times(65)
    ren = renderer_of(amd, dynamic_field(amd, sc, feat, requires_grad=False), Sc)
    ren.N_importance, ren.perturb, ren.samples = Sf, True, []
    draws, draw = [], ren._rand

    def recording(shape, device):
        draws.append(draw(shape, device))
        return draws[-1]
    ren._rand = recording
    torch.manual_seed(11)
    rgb, depth = ren.render(batch_of(sc, time))
    assert len(ren.samples) == 1 and [tuple(d.shape) for d in draws] == [(65, Sc), (65, Sf)]
    t_c, w_c, t_m = ren.samples[0]
    assert same(t_c, SR.stratified(sc["t"], draws[0].cpu()), "t_coarse")
    want, _ = SR.sample_importance(w_c.cpu(), t_c.cpu(), draws[1].cpu())
    assert same(t_m, want, "t_merged")
    figures, ok, res = {}, [], {}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        res[tag] = (dynamic_render(sc, feat, t_c.cpu(), time, 1, dtype)[2], dynamic_render(sc, feat, t_m.cpu(), time, 1, dtype))
    assert float(res["f64"][0].max()) > 0.1 and float(res["f64"][1][0].std()) > 1e-3
    ok.append(_allowed("weights_coarse", w_c, res["f64"][0], res["cpu32"][0], figures))
    ok.append(_allowed("rgb", rgb, res["f64"][1][0], res["cpu32"][1][0], figures))
    ok.append(_allowed("depth", depth, res["f64"][1][1], res["cpu32"][1][1], figures))
    record("importance_8_8_perturb", figures)
    assert all(ok), figures


def test_density_at_a_frame(amd):
    sc = R.scene(65, 64)
    feat = field_tables()
    field = dynamic_field(amd, sc, feat, requires_grad=False)
    pts = (torch.rand(257, 3, generator=torch.Generator().manual_seed(8)) - 0.5) * 4.0      # in [-2, 2]: some outside the box
    sigma = field.density(pts.cuda(), time=2)
    assert sigma.shape == (257, 1)
    x32 = R.points(pts, None, None, 1, None, 257, sc["frame"])
    _, xw = DR.deform(x32.numpy(), np.full(257, 2.0, dtype=np.float32), feat, np.float32)
    res = {}
    for tag, dtype in (("f64", torch.float64), ("cpu32", torch.float32)):
        params = R.cast_params(sc["params"], dtype)
        geo, _ = R.mlp(R.hash_forward(torch.from_numpy(xw), params["emb"], sc["offsets"], sc["scales"]), params["sw"], params["sb"])
        res[tag] = geo[:, 0]
    figures = {}
    assert _allowed("density", sigma[:, 0], res["f64"], res["cpu32"], figures), figures
    static_like = field.density(pts.cuda(), time=0.0)                             # frame 0 is the canonical frame
    params = R.cast_params(sc["params"], torch.float64)
    geo0, _ = R.mlp(R.hash_forward(x32, params["emb"], sc["offsets"], sc["scales"]), params["sw"], params["sb"])
    assert float((static_like[:, 0].double().cpu() - geo0[:, 0]).abs().max()) <= figures["density"]["allowance"]
    assert not torch.equal(static_like, sigma)


# ---- training --------------------------------------------------------------------------------------------------------------------------
def training_rays(amd, oracle, synthetic_sd):
    """1024 fixed rays of one teacher view at two frames of a moving scene: at frame 1 the scene is translated by SHIFT, which is the
    static teacher rendered with the rays shifted the other way.  -> (o, d, colours, time)."""
    from test_gpu_hashfield import training_rays as static_rays
    o, d, colors0 = static_rays(amd, oracle, synthetic_sd)
    teacher = amd.Network()
    teacher.load_state_dict(synthetic_sd, strict=True)
    teacher = teacher.cuda().eval()
    time = (torch.arange(1024, device="cuda") % 2).float()
    shift = torch.tensor([0.25, 0.0, 0.0], device="cuda")
    with torch.no_grad():
        colors1, _ = amd.Renderer(teacher).render({"rays_o": (o - shift)[None].contiguous(), "rays_d": d[None]})
    colors = torch.where((time == 1)[:, None], colors1, colors0).contiguous()
    return o, d, colors, time


def training_field(amd, seed=0):
    torch.manual_seed(seed)
    enc = amd.DNeRFNGP(2, reso=16, input_dim=3, num_levels=8, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=14)
    return amd.HashField((-2.0, -2.0, -2.0, 2.0, 2.0, 2.0), encoder=enc).cuda()


def run_fused(amd, rays, steps=40):
    from nerf_replication_amd.training import FusedAdam, train_step
    field = training_field(amd)
    ren = amd.HashRenderer(field)
    ren.N_samples = 64
    opt = FusedAdam(field.parameters(), lr=1e-2)
    assert len(opt.params) == 14                                                  # the three tables are in the one group
    o, d, colors, time = rays
    start = [f.detach().clone() for f in field.encoder.feat]
    losses = [float(train_step(ren, opt, o, d, colors, time=time)) for _ in range(steps)]
    return losses, max(float((f.detach() - s).abs().max()) for f, s in zip(field.encoder.feat, start))


def eager_delta(feat, x, t, T):
    """The reference's compute_delta in eager torch: grid_sample(align_corners=True) on (x_i, t / (T - 1))."""
    tn = (t / (T - 1))[:, None]
    coord = torch.stack([torch.cat([x[:, i:i + 1], tn], dim=-1) for i in range(3)])
    out = []
    for i in range(3):
        v = torch.nn.functional.grid_sample(feat[i], 2 * coord[:, None] - 1.0, align_corners=True)[:, :, 0]
        out.append(v.prod(dim=0).sum(dim=0))
    return torch.stack(out, dim=1)


def run_eager(amd, rays, steps=40):
    """The same field from the same initial state in eager torch on the same GPU (test_gpu_hashfield.run_eager with the warp: the
    grid_sample restatement, the canonical rule per ray, torch.clamp)."""
    field = training_field(amd)
    o, d, colors, time = rays
    dn = field.encoder
    t = torch.linspace(2.0, 6.0, 64, device="cuda")
    delta = torch.cat([t[1:] - t[:-1], torch.full((1,), 1e10, device="cuda")])
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    t_rows = time.repeat_interleave(64)
    losses = []

    def eager_mlp(net, x):
        for layer in net.layers[:-1]:
            x = torch.relu(layer(x))
        return net.layers[-1](x)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        pts = (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3)
        x01 = amd.hashgrid.normalize_to_bounds(pts, field.wbounds)
        warped = torch.clamp(x01 + eager_delta(dn.feat, x01, t_rows, dn.num_frames), 0.0, 1.0)
        x = torch.where((t_rows == 0)[:, None], x01, warped)
        geo = eager_mlp(field.sigma_net, dn.encoder(x, normalize=False))
        sh = R.sh4(d)
        rgb_raw = eager_mlp(field.color_net, torch.cat([geo, sh[:, None, :].expand(-1, 64, -1).reshape(-1, 16)], dim=1))
        alpha = 1.0 - torch.exp(-torch.relu(geo[:, 0].view(-1, 64)) * delta[None])
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), torch.clamp(1.0 - alpha, 1e-10, 1.0)], dim=1), dim=1)[:, :-1]
        w = T * alpha
        rgb = (w[..., None] * torch.sigmoid(rgb_raw.view(-1, 64, 3))).sum(1) + (1.0 - w.sum(1))[:, None]
        loss = torch.nn.functional.mse_loss(rgb, colors)
        loss.backward()
        torch.nn.utils.clip_grad_value_(field.parameters(), 40.0)
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_training_moves(amd, oracle, synthetic_sd):
    """40 train_step calls with FusedAdam(lr=1e-2) on 1024 fixed teacher rays of a two-frame scene: the loss falls, the tables move,
    and the loss ends at most K times where an eager-torch run of the same field from the same state ends.  K is twice the largest
    ratio (any fused run over any eager run) in five runs of each side, which tools/measure_deform_train_k.py makes and writes to
    profiles/deform_parity.json under "training_k" (hashfield_parity.json's convention); the test reads it there."""
    with open(DEFORM_JSON) as f:
        k = float(json.load(f)["training_k"]["k"])
    rays = training_rays(amd, oracle, synthetic_sd)
    fused, table_step = run_fused(amd, rays)
    eager = run_eager(amd, rays)
    print(f"fused {fused[0]:.5f} -> {fused[-1]:.5f}   eager {eager[0]:.5f} -> {eager[-1]:.5f}   ratio {fused[-1] / eager[-1]:.3f}  k {k}")
    record("training_moves", {"fused_first": fused[0], "fused_last": fused[-1], "eager_first": eager[0], "eager_last": eager[-1], "k": k})
    assert abs(fused[0] - eager[0]) <= 1e-4 * eager[0]                # the same field, the same rays
    assert fused[-1] < fused[0]
    assert fused[-1] <= k * eager[-1]
    assert table_step > 1e-3                                          # the tables were trained (Adam at lr 1e-2 moves them by that and more)
