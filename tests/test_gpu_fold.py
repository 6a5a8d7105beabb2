"""feature_linear folded into the views layer (csrc/nerf_layout.h kFold*, nerf_fold_f32_kernel): the fp32 kernels evaluate
    views = relu((Wv[:, :256] . Wf) . h7 + Wv[:, 256:] . dirs + (Wv[:, :256] . bf + bv))
with the product and the bias formed in float64 from the packed stream by nerf_pack_model, which writes them behind that stream
in the caller's buffer.  Checked here: the orientation and exactness of the fold, that the fold follows every repack, that the
training forward equals inference bit for bit, that streams share nothing (two models on two streams, a capture on a stream that
has never launched, more streams than any pool would hold, two models back to back on one stream), and the distance of the folded
chain to the float64 evaluation."""
import ctypes
import json
import os

import pytest
import torch

from gpu_common import amd, network  # noqa: F401

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLD_JSON = os.path.join(REPO, "profiles", "parity_fold.json")
MODELS = (("", "model"), ("fine", "model_fine"))


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 1, 3, generator=g) * 3.0 - 1.5)
    vd = torch.randn(n, 3, generator=g)
    return pts, vd / vd.norm(dim=-1, keepdim=True)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _forward_rays(amd, fn, net, o, d, t, save=False):
    """One of the ray-mode C-ABI forwards of the fine model on [n] rays x t.shape[1] depths -> raw [n, S, 4]."""
    L = amd._lib
    n, S = o.shape[0], t.shape[1]
    raw = torch.full((n, S, 4), float("nan"), device="cuda")
    args = [o, d, t, S, n, S, net.packed("fine"), raw]
    if save:
        args.append(torch.zeros(int(L.call("nerf_train_save_floats", n * S)), device="cuda"))
    L.call(fn, *args, 0)
    torch.cuda.synchronize()
    return raw


def test_fold_orientation_and_exactness(amd, oracle, synthetic_sd):
    """Two networks whose folds are the same numbers, exactly: A has a permutation matrix as feature_linear, a coarse-grained
    bias behind it and views weights on a 2^-10 grid (every product and sum of the fold is exact in float64); B has the
    permutation and the bias already multiplied into its views layer, and the identity as feature_linear.  Their outputs must
    agree bit for bit; a transposed or mis-ordered product in the fold kernel applies P^T (or permutes rows) and breaks it."""
    g = torch.Generator().manual_seed(11)
    sd_a = {k: v.clone() for k, v in synthetic_sd.items()}
    sd_b = {k: v.clone() for k, v in synthetic_sd.items()}
    for _, m in MODELS:
        perm = torch.randperm(256, generator=g)
        assert not torch.equal(perm, torch.argsort(perm)), "the permutation must differ from its inverse"
        P = torch.zeros(256, 256)
        P[torch.arange(256), perm] = 1.0
        bf = torch.randint(-128, 129, (256,), generator=g).float() / 64.0                      # multiples of 2^-6, |bf| <= 2
        wv = sd_a[f"{m}.views_linears.0.weight"].clone()
        wv[:, :256] = torch.round(wv[:, :256] * 1024.0) / 1024.0                              # multiples of 2^-10
        bv = sd_a[f"{m}.views_linears.0.bias"]
        sd_a[f"{m}.feature_linear.weight"], sd_a[f"{m}.feature_linear.bias"] = P, bf
        sd_a[f"{m}.views_linears.0.weight"] = wv
        wv_b = wv.clone()
        wv_b[:, :256] = (wv[:, :256].double() @ P.double()).float()                            # exact column permutation
        assert torch.equal(wv_b[:, :256].double(), wv[:, :256].double() @ P.double())
        sd_b[f"{m}.feature_linear.weight"], sd_b[f"{m}.feature_linear.bias"] = torch.eye(256), torch.zeros(256)
        sd_b[f"{m}.views_linears.0.weight"] = wv_b
        sd_b[f"{m}.views_linears.0.bias"] = (bv.double() + wv[:, :256].double() @ bf.double()).float()
    net_a, net_b = network(amd, sd_a, "f32", train=False), network(amd, sd_b, "f32", train=False)
    pts, vd = _points(35, 3)                                                                   # a ragged tile
    with torch.no_grad():
        for model, _ in MODELS:
            ra, rb = net_a(pts.cuda(), vd.cuda(), None, model), net_b(pts.cuda(), vd.cuda(), None, model)
            assert torch.isfinite(ra).all() and ra[..., :3].abs().max() > 0
            assert torch.equal(_bits(ra), _bits(rb)), model
    o, d = oracle.seeded_rays(3, 5)
    t = torch.linspace(2.0, 6.0, 64)[None].expand(3, 64).contiguous()
    ra = _forward_rays(amd, "nerf_mlp_forward_rays", net_a, o.cuda(), d.cuda(), t.cuda())
    rb = _forward_rays(amd, "nerf_mlp_forward_rays", net_b, o.cuda(), d.cuda(), t.cuda())
    assert torch.isfinite(ra).all() and torch.equal(_bits(ra), _bits(rb))


def test_no_stale_fold_after_in_place_updates(amd, oracle, synthetic_sd):
    """The fold follows the repack: after an in-place update of each tensor it depends on, a render and a points forward
    equal those of a freshly constructed network with the same state dict."""
    net = network(amd, synthetic_sd, "f32", train=False)
    o, d = oracle.seeded_rays(64, 9)
    batch = {"rays_o": o[None].cuda(), "rays_d": d[None].cuda()}
    pts, vd = _points(35, 4)
    pts, vd = pts.cuda(), vd.cuda()
    g = torch.Generator().manual_seed(2)
    seen = []
    with torch.no_grad():
        for name in ("feature_linear.weight", "feature_linear.bias", "views_linears.0.weight", "views_linears.0.bias"):
            for sub in (net.model, net.model_fine):
                p = dict(sub.named_parameters())[name]
                p.add_((torch.randn(p.shape, generator=g) * 0.05).cuda())
            fresh = network(amd, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, "f32", train=False)
            rgb, dep = amd.Renderer(net).render(batch)
            rgb_f, dep_f = amd.Renderer(fresh).render(batch)
            assert torch.equal(_bits(rgb), _bits(rgb_f)) and torch.equal(_bits(dep), _bits(dep_f)), name
            for model, _ in MODELS:
                assert torch.equal(_bits(net(pts, vd, None, model)), _bits(fresh(pts, vd, None, model))), (name, model)
            seen.append(rgb.clone())
    assert all(not torch.equal(a, b) for a, b in zip(seen, seen[1:])), "an update did not reach the image"


@pytest.mark.parametrize("family", ["base", "sharp"])
def test_save_forward_equals_inference(amd, golden, family_sd, family):
    """The training (SAVE) forward forms the views layer with the instructions of the inference kernels: raw bit-equal at the
    C ABI (tiles with and without density) and through Network.forward in .train() and .eval()."""
    g = golden(f"render_family_{family}.npz")
    net = network(amd, family_sd(family), "f32", train=False)
    n = 67
    o, d = g["pin_rays_o"][:n].cuda().contiguous(), g["pin_rays_d"][:n].cuda().contiguous()
    t = g["pin_t_sorted"][:n].cuda().contiguous()
    assert t.shape[1] == 192
    inf = _forward_rays(amd, "nerf_mlp_forward_rays_for_compositing", net, o, d, t)
    sav = _forward_rays(amd, "nerf_mlp_forward_rays_save_for_compositing", net, o, d, t, save=True)
    assert torch.isfinite(inf).all() and torch.equal(_bits(inf), _bits(sav))
    dead = (inf[..., 3] <= 0).reshape(n, 6, 32).all(-1)
    assert (~dead).any() and (family == "base" or dead.any())
    full = _forward_rays(amd, "nerf_mlp_forward_rays", net, o, d, t)
    assert torch.equal(_bits(full), _bits(_forward_rays(amd, "nerf_mlp_forward_rays_save", net, o, d, t, save=True)))
    pts, vd = _points(35, 6)
    pts, vd = pts.cuda(), vd.cuda()
    for model, _ in MODELS:
        with torch.no_grad():
            ev = net(pts, vd, None, model)
        net.train()
        tr = net(pts, vd, None, model)
        net.eval()
        assert tr.requires_grad and torch.equal(_bits(ev), _bits(tr.detach())), model


def test_two_streams_two_models(amd, oracle, family_sd):
    """Nothing is shared between streams (the fold lies in each model's own packed buffer): two models rendering on two streams
    at once each get their own result."""
    nets = [network(amd, family_sd(f), "f32", train=False) for f in ("base", "sharp")]
    o, d = oracle.seeded_rays(2048, 13)
    batch = {"rays_o": o[None].cuda(), "rays_d": d[None].cuda()}
    with torch.no_grad():
        want = [amd.Renderer(n).render(batch) for n in nets]
        torch.cuda.synchronize()
        assert not torch.equal(want[0][0], want[1][0])
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        got = []
        for _ in range(3):
            for n, s in zip(nets, streams):
                with torch.cuda.stream(s):
                    got.append(amd.Renderer(n).render(batch))
        torch.cuda.synchronize()
    for i, (rgb, dep) in enumerate(got):
        assert torch.equal(_bits(rgb), _bits(want[i % 2][0])) and torch.equal(_bits(dep), _bits(want[i % 2][1])), i


def _points_forward(amd, net, pts, vd, raw):
    """nerf_mlp_forward of the fine model, fp32, enqueued on the current stream; everything preallocated."""
    amd._lib.call("nerf_mlp_forward", pts, vd, pts.shape[0], pts.shape[1], net.packed("fine"), raw, 0)


def _eager(amd, net, pts, vd):
    raw = torch.full((pts.shape[0], pts.shape[1], 4), float("nan"), device="cuda")
    _points_forward(amd, net, pts, vd, raw)
    torch.cuda.synchronize()
    assert torch.isfinite(raw).all() and raw[..., :3].abs().max() > 0
    return raw


def test_capture_on_a_stream_that_never_launched(amd, synthetic_sd):
    """A forward needs nothing but its arguments, so the first thing a new stream ever does can be a capture: one
    nerf_mlp_forward of 35 points (a ragged tile), model packed and tensors allocated beforehand, captured as a one-node graph,
    replayed, bit-equal to the eager call."""
    net = network(amd, synthetic_sd, "f32", train=False)
    pts, vd = _points(35, 8)
    pts, vd = pts.cuda(), vd.cuda()
    want = _eager(amd, net, pts, vd)
    raw = torch.full_like(want, float("nan"))
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _points_forward(amd, net, pts, vd, raw)                    # the current stream is `side` here
    torch.cuda.synchronize()
    assert torch.isnan(raw).all()                    # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(raw), _bits(want))


def test_65_streams(amd, synthetic_sd):
    """The same forward on 65 distinct streams, one after another: every call succeeds and gives the same bits (no per-stream
    resource exists that could run out).  The streams come from the HIP runtime the library is linked against (torch hands out
    32 pooled handles per priority)."""
    lib, L = amd._lib.load(), amd._lib
    create, destroy = lib.hipStreamCreate, lib.hipStreamDestroy
    create.restype, create.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p)]
    destroy.restype, destroy.argtypes = ctypes.c_int, [ctypes.c_void_p]
    net = network(amd, synthetic_sd, "f32", train=False)
    pts, vd = _points(35, 8)
    pts, vd = pts.cuda(), vd.cuda()
    want = _eager(amd, net, pts, vd)
    raws = torch.full((65,) + tuple(want.shape), float("nan"), device="cuda")
    torch.cuda.synchronize()
    streams = []
    try:
        for i in range(65):
            h = ctypes.c_void_p()
            assert create(ctypes.byref(h)) == 0 and h.value
            streams.append(h)
            # a raw stream handle, which call() cannot take: the direct path
            L.check(lib.nerf_mlp_forward(L.ptr(pts), L.ptr(vd), pts.shape[0], pts.shape[1], net.packed("fine").data_ptr(), L.ptr(raws[i]), 0, h),
                    "nerf_mlp_forward")
        torch.cuda.synchronize()
    finally:
        for h in streams:
            assert destroy(h) == 0
    assert len({h.value for h in streams}) == 65
    assert all(torch.equal(_bits(r), _bits(want)) for r in raws)


def test_two_models_back_to_back_on_one_stream(amd, family_sd):
    """"base" and "sharp" on one stream with no synchronisation in between: each returns its own eager result."""
    nets = [network(amd, family_sd(f), "f32", train=False) for f in ("base", "sharp")]
    pts, vd = _points(35, 8)
    pts, vd = pts.cuda(), vd.cuda()
    want = [_eager(amd, n, pts, vd) for n in nets]
    assert not torch.equal(want[0], want[1])
    raws = [torch.full_like(w, float("nan")) for w in want]
    torch.cuda.synchronize()
    for n, r in zip(nets, raws):
        _points_forward(amd, n, pts, vd, r)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(r), _bits(w)) for r, w in zip(raws, want))


def _chan_err(got, ref):
    """largest channel error relative to the channel's largest magnitude"""
    scale = ref.reshape(-1, 3).abs().max(0).values.clamp_min(1e-6)
    return ((got.double() - ref).abs().reshape(-1, 3).max(0).values / scale).max().item()


@pytest.mark.parametrize("family", ["base", "sharp", "white", "trained"])
def test_folded_colours_are_as_close_to_float64_as_the_reference(amd, oracle, family_sd, family):
    """Pre-activation colours of 4 096 random points against the oracle's float64 evaluation, judged against the oracle's own
    fp32-to-float64 distance (the form of tests/test_gpu_train_steps.py): at most 3 x that floor + 2e-7 of the channel maximum
    (3 fp32 ulps of it, 3 x 2^-24: the three roundings that bring a pre-activation colour out of its fp32 chain -- the rgb
    head's sum, the lane-half combine and the bias -- which the floor of a lucky family may not show).  A fold accumulated in
    fp32 instead of float64 would add about sqrt(256) x 2^-24 = 1e-6 to the views layer and miss this.  Measured ratios are
    recorded in profiles/parity_fold.json (CPU model of the folded chain: 1.0 in every family; MI355X: 0.78 .. 1.25)."""
    sd = family_sd(family)
    net = network(amd, sd, "f32", train=False)
    pts, vd = _points(4096, 21)
    ratios = {}
    for model, prefix in MODELS:
        with torch.no_grad():
            hip = net(pts.cuda(), vd.cuda(), None, model).cpu()
        ref64 = oracle.network_forward(sd, pts, vd, model, 1 << 16, torch.float64)      # (rounded to fp32 at the very end)
        ref32 = oracle.network_forward(sd, pts, vd, model, 1 << 16, torch.float32)
        truth = ref64[..., :3].double()
        floor = _chan_err(ref32[..., :3], truth)
        err = _chan_err(hip[..., :3], truth)
        ratios[prefix] = {"hip_err": err, "reference_fp32_err": floor, "ratio": err / max(floor, 1e-30)}
        print(f"{family}/{prefix}: HIP {err:.3e}  reference fp32 {floor:.3e}  ratio {err / max(floor, 1e-30):.2f}")
    rec = {}
    if os.path.exists(FOLD_JSON):
        with open(FOLD_JSON) as f:
            rec = json.load(f)
    rec.setdefault("colour_vs_float64", {})[family] = ratios
    with open(FOLD_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    for prefix, r in ratios.items():
        assert r["hip_err"] <= 3.0 * r["reference_fp32_err"] + 2e-7, (family, prefix, r)
